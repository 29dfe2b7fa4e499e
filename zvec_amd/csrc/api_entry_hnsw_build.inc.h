// api_entry_hnsw_build.inc.h — C ABI entry points: building an HNSW graph from rows on the device (zvec_hip_hnsw_build*; inside
// extern "C").  Device code: zvk_hnsw_build.hip.h; host planning: host/hnsw_add_plan.h.  Rows in, searchable graph out: the handle of
// api_entry_hnsw.inc.h then answers search, info, export and get_vectors as after a load.  The rule is DESIGN §3c "Building":
// HnswAlgorithm::add_node, update_neighbors and reverse_update_neighbors (hnsw_algorithm.cc:31-81, 394-515) applied in rounds.
// hnsw_run_rounds is shared with the append (api_entry_hnsw_add.inc.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

static_assert(HNSW_PLAN_MAX_LEVEL == HNSW_BUILD_MAX_LEVEL && HNSW_PLAN_MAX_EF == HNSW_MAX_EF && HNSW_PLAN_MAX_M0 == HNSW_BUILD_MAX_M0 &&
              HNSW_PLAN_MAX_M == HNSW_BUILD_MAX_M && HNSW_PLAN_C_LDS == HNSW_C_LDS, "host/hnsw_add_plan.h restates the kernels' limits");

// HnswAlgorithm::get_random_level (hnsw_algorithm.h) in integer arithmetic
int zvec_hip_hnsw_build_levels(uint64_t n, uint32_t scaling_factor, uint64_t seed, uint32_t *out_levels) {
  return hnsw_levels_range(0, n, scaling_factor, seed, out_levels);
}

namespace {
struct HnswEvent {
  hipEvent_t e = nullptr;
  ~HnswEvent() { if (e) (void)hipEventDestroy(e); }
};
// what a run of rounds did
struct HnswRoundsDone {
  uint32_t slices = 0, one = 0;                  // the most slices of a round's insert phase; rounds on the one-node path
  double insert_ms = 0, reverse_ms = 0;
  uint64_t dists = 0, requests = 0, prunes = 0;
};
}  // namespace

// The rounds of `plan` on the arrays `arr` (sized and initialised for every node of the plan; stride of the upper table max_level) with
// the parameters q.  lv / req_off: levels and request offsets of the nodes from node_base on (host/hnsw_add_plan.h).  A round of one
// node applies its requests straight from the round buffer (hnsw_reverse_one_kernel); a round of more sorts and groups them first.
// The caller holds h->mu, the default context's mutex and h->rw exclusively, and has synchronised the device.
static int hnsw_run_rounds(zvec_hip_hnsw_s *h, const zvec_hip_hnsw_s::Arrays &arr, uint32_t max_level, const zvec_hip_hnsw_build_params &q,
                           uint32_t node_base, const std::vector<uint32_t> &lv, const std::vector<HnswRound> &plan,
                           const std::vector<uint64_t> &req_off, const HnswRoundsNeed &need, uint64_t budget, HnswRoundsDone &done) {
  if (plan.empty()) return 0;
  zvec_hip_ctx_s *c = h->defctx;
  hipStream_t s = c->cur;
  Scoped<uint32_t> d_levels, gstart, ngroups;
  Scoped<uint64_t> d_req_off, req_a, req_b;
  Scoped<unsigned long long> counters;
  Scoped<unsigned char> sort_tmp;
  ZRET(upload(d_levels, lv.data(), lv.size()));
  ZRET(upload(d_req_off, req_off.data(), req_off.size()));
  ZRET(req_a.alloc(need.max_slots));
  ZRET(counters.alloc(3));
  ZCHK(hipMemset(counters, 0, 3 * sizeof(unsigned long long)));
  size_t tmp_bytes = 0;
  if (need.multi) {
    ZRET(req_b.alloc(need.max_slots));
    ZRET(gstart.alloc(need.max_slots));
    ZRET(ngroups.alloc(1));
    ZCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, req_a.p, req_b.p, (int)need.max_slots, 0, 64, s));
    ZRET(sort_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
  }
  ZRET(c->hnsw_ws.ensure((size_t)need.max_ws));
  HnswEvent ev[3];
  for (HnswEvent &e : ev) ZCHK(hipEventCreate(&e.e));

  HnswBuildArgs b{};
  HnswArgs &a = b.g;
  a.rows = arr.rows; a.keys = arr.keys; a.nbr0 = arr.nbr0; a.cnt0 = arr.cnt0; a.upper_of = arr.upper_of;
  a.nbr_up = arr.nbr_up; a.cnt_up = arr.cnt_up;
  a.n = plan.back().end; a.dim = h->dim; a.dpad = h->dpad; a.m0 = q.m0; a.m = q.m; a.max_level = max_level;
  a.ip = h->metric == ZVEC_HIP_METRIC_IP ? 1 : 0;
  a.ef = q.ef_construction; a.max_scan = 0xffffffffu; a.threshold = 0.f;
  b.nbr0 = arr.nbr0; b.cnt0 = arr.cnt0; b.nbr_up = arr.nbr_up; b.cnt_up = arr.cnt_up;
  b.node_base = node_base; b.levels = d_levels; b.req_off = d_req_off; b.req = req_a;
  b.prune_cnt = q.prune_cnt; b.min_neighbors = q.min_neighbors; b.counters = counters;
  const size_t lds_ins = hnsw_insert_lds_bytes(a.dpad, a.ef), lds_rev = hnsw_reverse_lds_bytes(a.dpad);
  for (const HnswRound &r : plan) {
    const bool spill = r.first > HNSW_C_LDS;
    a.entry = r.entry; a.ccap = r.first; a.vis_words = (r.first + 31) / 32;
    b.round_first = r.first; b.top = r.top; b.req_base = req_off[r.first - node_base];
    const uint32_t slice = hnsw_round_slice(r, budget);
    a.cand_ws = spill ? c->hnsw_ws.as<uint64_t>() : nullptr;
    a.visited = reinterpret_cast<uint32_t *>(c->hnsw_ws.as<uint64_t>() + (spill ? (size_t)slice * a.ccap : 0));
    ZCHK(hipEventRecord(ev[0].e, s));
    uint32_t slices = 0;
    for (uint32_t f = r.first; f < r.end; f += slice, ++slices) {     // (the graph is frozen: a slice sees what every slice sees)
      b.first = f;
      hipLaunchKernelGGL(h->f16() ? hnsw_insert_kernel<true> : hnsw_insert_kernel<false>, dim3(std::min(slice, r.end - f)), dim3(64), lds_ins, s, b);
      ZCHK(hipGetLastError());
    }
    done.slices = std::max(done.slices, slices);
    ZCHK(hipEventRecord(ev[1].e, s));
    const uint64_t slots = req_off[r.end - node_base] - req_off[r.first - node_base];
    if (r.end - r.first == 1) {
      // the reverse phase of one node: every used request word is a (level, target) group of its own
      hipLaunchKernelGGL(h->f16() ? hnsw_reverse_one_kernel<true> : hnsw_reverse_one_kernel<false>, dim3((uint32_t)std::min<uint64_t>(slots, 4096)), dim3(64), lds_rev, s, b, slots);
      ZCHK(hipGetLastError());
      ++done.one;
    } else {
      // the reverse phase: group the round's requests by (level, target, source), then one wave per (level, target)
      ZCHK(hipcub::DeviceRadixSort::SortKeys(sort_tmp.p, tmp_bytes, req_a.p, req_b.p, (int)slots, 0, 64, s));
      ZCHK(hipMemsetAsync(ngroups, 0, 4, s));
      hipLaunchKernelGGL(hnsw_groups_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, req_b.p, slots, gstart.p, ngroups.p);
      ZCHK(hipGetLastError());
      hipLaunchKernelGGL(h->f16() ? hnsw_reverse_kernel<true> : hnsw_reverse_kernel<false>, dim3((uint32_t)std::min<uint64_t>(slots, 4096)),
                         dim3(64), lds_rev, s, b, req_b.p, slots, gstart.p, ngroups.p);
      ZCHK(hipGetLastError());
    }
    ZCHK(hipEventRecord(ev[2].e, s));
    ZCHK(hipEventSynchronize(ev[2].e));
    float ms = 0.f;
    ZCHK(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
    done.insert_ms += ms;
    ZCHK(hipEventElapsedTime(&ms, ev[1].e, ev[2].e));
    done.reverse_ms += ms;
  }
  ZCHK(hipStreamSynchronize(s));
  unsigned long long cnt[3];
  ZCHK(hipMemcpy(cnt, counters, sizeof(cnt), hipMemcpyDeviceToHost));
  done.dists = cnt[0]; done.requests = cnt[1]; done.prunes = cnt[2];
  return 0;
}

// the caller holds h->mu, the default context's mutex and h->rw exclusively; rows: [n][dim], on the device or on the host
static int hnsw_build_locked(zvec_hip_hnsw_s *h, uint64_t n64, const void *rows, bool rows_on_device, const uint64_t *keys,
                             const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  zvec_hip_hnsw_build_params q{};
  ZRET(hnsw_add_params(p, zvec_hip_hnsw_build_params(), 0, 0, 0, q));      // (a build remembers nothing and finds no graph)
  if (h->dim > HNSW_MAX_DIM) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (n64 >= HNSW_PLAN_MAX_NODES) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  if (n64 && !rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const uint32_t n = (uint32_t)n64;
  std::vector<uint32_t> lv;
  ZRET(hnsw_add_levels(0, n, levels, q, lv));
  const uint32_t round_div = (uint32_t)ropts().hnsw_build_round_div.load(std::memory_order_relaxed);
  const uint32_t round_max = (uint32_t)ropts().hnsw_build_round_max.load(std::memory_order_relaxed);
  std::vector<HnswRound> plan;
  std::vector<uint64_t> req_off;
  uint32_t entry = 0, top = 0;
  hnsw_plan_rounds(0, lv.data(), n, round_div, round_max, q.m0, q.m, entry, top, plan, req_off);
  std::vector<uint32_t> upper_of(n);
  const HnswAddShape shape = hnsw_add_shape(0, 0, lv.data(), n, upper_of.data());
  const uint32_t max_level = shape.stride, n_upper = shape.n_upper;
  const bool up = max_level >= 1;
  const uint64_t budget = (uint64_t)ropts().hnsw_ws_bytes.load(std::memory_order_relaxed);
  const HnswRoundsNeed need = hnsw_rounds_need(plan, req_off, 0, budget);
  if (need.max_slots >= (1ull << 31)) return ZVEC_HIP_ERR_UNSUPPORTED;     // (group starts are 32-bit, the sort counts in int)

  zvec_hip_ctx_s *c = h->defctx;
  ZCHK(hipDeviceSynchronize());                  // (searches enqueued on other contexts have finished with the old arrays)
  zvec_hip_hnsw_s::Arrays arr;
  zvec_hip_hnsw_build_info info{};
  info.rounds = (uint32_t)plan.size();
  info.top = top;
  info.entry_point = entry;
  if (n) {
    ZRET(arr.rows.alloc((size_t)n * h->pad_bytes()));
    ZRET(arr.keys.alloc(n));
    ZRET(arr.cnt0.alloc(n));
    ZRET(arr.nbr0.alloc(std::max<size_t>((size_t)n * q.m0, 1)));
    if (h->dpad != h->dim) ZCHK(hipMemset(arr.rows, 0, (size_t)n * h->pad_bytes()));
    ZCHK(hipMemcpy2D(arr.rows, h->pad_bytes(), rows, h->row_bytes(), h->row_bytes(), n,
                     rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (keys) {
      ZCHK(hipMemcpy(arr.keys, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    } else {
      std::vector<uint64_t> id(n);
      for (uint32_t i = 0; i < n; ++i) id[i] = i;
      ZCHK(hipMemcpy(arr.keys, id.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    ZCHK(hipMemset(arr.cnt0, 0, (size_t)n * 4));
    ZCHK(hipMemset(arr.nbr0, 0, (size_t)n * q.m0 * 4));
  }
  const size_t up_slots = (size_t)n_upper * max_level;
  if (up) {
    ZRET(arr.upper_of.alloc(n));
    ZRET(arr.cnt_up.alloc(up_slots));
    ZRET(arr.nbr_up.alloc(up_slots * q.m));
    ZCHK(hipMemcpy(arr.upper_of, upper_of.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    ZCHK(hipMemset(arr.cnt_up, 0, up_slots * 4));
    ZCHK(hipMemset(arr.nbr_up, 0, up_slots * q.m * 4));
  }
  // (a list keeps nothing behind its count: the lists start zeroed and a prune zeroes what it empties)
  HnswRoundsDone done;
  ZRET(hnsw_run_rounds(h, arr, max_level, q, 0, lv, plan, req_off, need, budget, done));
  info.slices = done.slices; info.insert_ms = done.insert_ms; info.reverse_ms = done.reverse_ms;
  info.dists = done.dists; info.requests = done.requests; info.prunes = done.prunes;
  std::swap(h->arr, arr);                        // the old arrays go with the local
  h->n = n; h->m0 = q.m0; h->m = up ? q.m : 0; h->max_level = up ? max_level : 0; h->n_upper = up ? n_upper : 0;
  h->entry = n ? entry : 0;
  h->cap_rows = n; h->cap_upper = up ? n_upper : 0;
  h->params = q;
  h->loaded = true;
  h->built = true;
  h->binfo = info;
  c->hnsw_count = 0;
  return 0;
}

static int hnsw_build_entry(zvec_hip_hnsw_t h, uint64_t n, const void *rows, bool rows_on_device, const uint64_t *keys,
                            const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::unique_lock<FairSharedMutex> w(h->rw);
  return hnsw_build_locked(h, n, rows, rows_on_device, keys, p, levels);
}

// HnswBuilder::train + build (hnsw_builder.cc): every row goes through HnswAlgorithm::add_node (hnsw_algorithm.cc:31-81)
int zvec_hip_hnsw_build(zvec_hip_hnsw_t h, uint64_t n, const void *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                        const uint32_t *levels) {
  return hnsw_build_entry(h, n, rows, false, keys, p, levels);
}

// the same behind a holder whose rows are in device memory already
int zvec_hip_hnsw_build_dev(zvec_hip_hnsw_t h, uint64_t n, const void *d_rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                            const uint32_t *levels) {
  return hnsw_build_entry(h, n, d_rows, true, keys, p, levels);
}

// HnswBuilder::stats() (hnsw_builder.h) for the last build: what was done and how long the device took
int zvec_hip_hnsw_last_build_info(zvec_hip_hnsw_t h, zvec_hip_hnsw_build_info *out) {
  if (!h || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->built) return ZVEC_HIP_ERR_NO_READY;
  *out = h->binfo;
  return 0;
}
