// api_entry_hnsw_build.inc.h — C ABI entry points: building an HNSW graph from rows on the device (zvec_hip_hnsw_build*; inside
// extern "C").  Device code: zvk_hnsw_build.hip.h.  Rows in, searchable graph out: the handle of api_entry_hnsw.inc.h then answers
// search, info, export and get_vectors as after a load.  The rule is DESIGN §3c "Building": HnswAlgorithm::add_node,
// update_neighbors and reverse_update_neighbors (hnsw_algorithm.cc:31-81, 394-515) applied in rounds.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// HnswAlgorithm::get_random_level (hnsw_algorithm.h) in integer arithmetic
int zvec_hip_hnsw_build_levels(uint64_t n, uint32_t scaling_factor, uint64_t seed, uint32_t *out_levels) {
  if (n && !out_levels) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (scaling_factor < 5 || scaling_factor > 1000) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  // thr[k - 1] = ceil(2^53 / sf^k): r * sf^k < 2^53 <=> r < thr[k - 1]; once sf^k >= 2^53 only r == 0 passes
  uint64_t thr[HNSW_BUILD_MAX_LEVEL];
  uint64_t pw = 1;
  for (uint32_t k = 0; k < HNSW_BUILD_MAX_LEVEL; ++k) {
    if (pw < (1ull << 53)) pw *= scaling_factor;
    thr[k] = ((1ull << 53) + pw - 1) / pw;
  }
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t z = seed + i * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    const uint64_t r = (z ^ (z >> 31)) >> 11;
    uint32_t level = 0;
    while (level < HNSW_BUILD_MAX_LEVEL && r < thr[level]) ++level;
    out_levels[i] = level;
  }
  return 0;
}

namespace {
struct HnswRound { uint32_t first, end, entry, top; };
struct HnswEvent {
  hipEvent_t e = nullptr;
  ~HnswEvent() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace

// the rounds after the seed node 0 (DESIGN §3c "Building"), and the first request slot of every node: a node has m0 slots for
// level 0 and m for every level it is searched on above it
static void hnsw_build_plan(const std::vector<uint32_t> &lv, uint32_t round_div, uint32_t round_max, uint32_t m0, uint32_t m,
                            std::vector<HnswRound> &plan, std::vector<uint64_t> &req_off, uint32_t &entry, uint32_t &top) {
  const uint32_t n = (uint32_t)lv.size();
  req_off.assign((size_t)n + 1, 0);
  entry = 0;
  top = n ? lv[0] : 0;
  uint32_t s = 1;
  if (n) req_off[1] = 0;
  while (s < n) {
    uint32_t e;
    const bool own = lv[s] > top;                  // add_node:73-78: the node becomes the entry point after its round
    if (own) {
      e = s + 1;
    } else {
      const uint32_t size = round_div == 0 ? 1u : std::min(std::max(s / round_div, 1u), round_max);
      e = (uint32_t)std::min<uint64_t>((uint64_t)s + size, n);
      for (uint32_t j = s + 1; j < e; ++j)
        if (lv[j] > top) { e = j; break; }
    }
    plan.push_back({s, e, entry, top});
    for (uint32_t i = s; i < e; ++i) req_off[(size_t)i + 1] = req_off[i] + m0 + (uint64_t)std::min(lv[i], top) * m;
    if (own) { entry = s; top = lv[s]; }
    s = e;
  }
}

// the caller holds h->mu, the default context's mutex and h->rw exclusively; rows: [n][dim], on the device or on the host
static int hnsw_build_locked(zvec_hip_hnsw_s *h, uint64_t n64, const float *rows, bool rows_on_device, const uint64_t *keys,
                             const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  zvec_hip_hnsw_build_params q{};
  if (p) q = *p;
  if (q.m == 0) q.m = 50;
  if (q.m0 == 0) q.m0 = 2 * q.m;
  if (q.ef_construction == 0) q.ef_construction = 500;
  if (q.prune_cnt == 0) q.prune_cnt = q.m;
  if (q.scaling_factor == 0) q.scaling_factor = q.m;
  if (q.ef_construction > HNSW_MAX_EF || q.m0 > HNSW_BUILD_MAX_M0 || q.m > HNSW_BUILD_MAX_M || h->dim > HNSW_MAX_DIM)
    return ZVEC_HIP_ERR_UNSUPPORTED;
  if (q.min_neighbors > std::min(q.m, q.m0)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n64 >= 0xfffffff0ull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  if (n64 && !rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const uint32_t n = (uint32_t)n64;
  std::vector<uint32_t> lv(n);
  if (levels) {
    for (uint32_t i = 0; i < n; ++i) {
      if (levels[i] > HNSW_BUILD_MAX_LEVEL) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
      lv[i] = levels[i];
    }
  } else {
    ZRET(zvec_hip_hnsw_build_levels(n, q.scaling_factor, q.seed, lv.data()));
  }
  const uint32_t round_div = (uint32_t)ropts().hnsw_build_round_div.load(std::memory_order_relaxed);
  const uint32_t round_max = (uint32_t)ropts().hnsw_build_round_max.load(std::memory_order_relaxed);
  std::vector<HnswRound> plan;
  std::vector<uint64_t> req_off;
  uint32_t entry = 0, top = 0;
  hnsw_build_plan(lv, round_div, round_max, q.m0, q.m, plan, req_off, entry, top);
  uint32_t max_level = 0, n_upper = 0;
  std::vector<uint32_t> upper_of(n, IDX_NONE);
  for (uint32_t i = 0; i < n; ++i) {
    max_level = std::max(max_level, lv[i]);
    if (lv[i] >= 1) upper_of[i] = n_upper++;
  }
  const bool up = max_level >= 1;
  // what one round needs at most: request slots, and the workspace of one slice of its insert phase
  const uint64_t budget = (uint64_t)ropts().hnsw_ws_bytes.load(std::memory_order_relaxed);
  uint64_t max_slots = 0, max_ws = 0;
  for (const HnswRound &r : plan) {
    max_slots = std::max(max_slots, req_off[r.end] - req_off[r.first]);
    const uint64_t per = (uint64_t)((r.first + 31) / 32) * 4 + (r.first > HNSW_C_LDS ? (uint64_t)r.first * 8 : 0);
    const uint64_t slice = std::max<uint64_t>(1, std::min<uint64_t>(r.end - r.first, budget / per));
    max_ws = std::max(max_ws, slice * per);
  }
  if (max_slots >= (1ull << 31)) return ZVEC_HIP_ERR_UNSUPPORTED;     // (group starts are 32-bit, the sort counts in int)

  zvec_hip_ctx_s *c = h->defctx;
  hipStream_t s = c->cur;
  ZCHK(hipDeviceSynchronize());                  // (searches enqueued on other contexts have finished with the old arrays)
  zvec_hip_hnsw_s::Arrays arr;
  zvec_hip_hnsw_build_info info{};
  info.rounds = (uint32_t)plan.size();
  info.top = top;
  info.entry_point = entry;
  if (n) {
    ZRET(arr.rows.alloc((size_t)n * h->dpad));
    ZRET(arr.keys.alloc(n));
    ZRET(arr.cnt0.alloc(n));
    ZRET(arr.nbr0.alloc(std::max<size_t>((size_t)n * q.m0, 1)));
    if (h->dpad != h->dim) ZCHK(hipMemset(arr.rows, 0, (size_t)n * h->dpad * 4));
    ZCHK(hipMemcpy2D(arr.rows, (size_t)h->dpad * 4, rows, (size_t)h->dim * 4, (size_t)h->dim * 4, n,
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
  if (!plan.empty()) {
    Scoped<uint32_t> d_levels, gstart, ngroups;
    Scoped<uint64_t> d_req_off, req_a, req_b;
    Scoped<unsigned long long> counters;
    Scoped<unsigned char> sort_tmp;
    ZRET(upload(d_levels, lv.data(), n));
    ZRET(upload(d_req_off, req_off.data(), (size_t)n + 1));
    ZRET(req_a.alloc(max_slots));
    ZRET(req_b.alloc(max_slots));
    ZRET(gstart.alloc(max_slots));
    ZRET(ngroups.alloc(1));
    ZRET(counters.alloc(3));
    ZCHK(hipMemset(counters, 0, 3 * sizeof(unsigned long long)));
    size_t tmp_bytes = 0;
    ZCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, req_a.p, req_b.p, (int)max_slots, 0, 64, s));
    ZRET(sort_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    ZRET(c->hnsw_ws.ensure((size_t)max_ws));
    HnswEvent ev[3];
    for (HnswEvent &e : ev) ZCHK(hipEventCreate(&e.e));

    HnswBuildArgs b{};
    HnswArgs &a = b.g;
    a.rows = arr.rows; a.keys = arr.keys; a.nbr0 = arr.nbr0; a.cnt0 = arr.cnt0; a.upper_of = arr.upper_of;
    a.nbr_up = arr.nbr_up; a.cnt_up = arr.cnt_up;
    a.n = n; a.dim = h->dim; a.dpad = h->dpad; a.m0 = q.m0; a.m = q.m; a.max_level = max_level;
    a.ip = h->metric == ZVEC_HIP_METRIC_IP ? 1 : 0;
    a.ef = q.ef_construction; a.max_scan = 0xffffffffu; a.threshold = 0.f;
    b.nbr0 = arr.nbr0; b.cnt0 = arr.cnt0; b.nbr_up = arr.nbr_up; b.cnt_up = arr.cnt_up;
    b.levels = d_levels; b.req_off = d_req_off; b.req = req_a;
    b.prune_cnt = q.prune_cnt; b.min_neighbors = q.min_neighbors; b.counters = counters;
    const size_t lds_ins = hnsw_insert_lds_bytes(a.dpad, a.ef), lds_rev = hnsw_reverse_lds_bytes(a.dpad);
    for (const HnswRound &r : plan) {
      const uint32_t size = r.end - r.first;
      const bool spill = r.first > HNSW_C_LDS;
      a.entry = r.entry; a.ccap = r.first; a.vis_words = (r.first + 31) / 32;
      b.round_first = r.first; b.top = r.top; b.req_base = req_off[r.first];
      const uint64_t per = (uint64_t)a.vis_words * 4 + (spill ? (uint64_t)a.ccap * 8 : 0);
      const uint32_t slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(size, budget / per));
      a.cand_ws = spill ? c->hnsw_ws.as<uint64_t>() : nullptr;
      a.visited = reinterpret_cast<uint32_t *>(c->hnsw_ws.as<uint64_t>() + (spill ? (size_t)slice * a.ccap : 0));
      ZCHK(hipEventRecord(ev[0].e, s));
      uint32_t slices = 0;
      for (uint32_t f = r.first; f < r.end; f += slice, ++slices) {     // (the graph is frozen: a slice sees what every slice sees)
        b.first = f;
        hipLaunchKernelGGL(hnsw_insert_kernel, dim3(std::min(slice, r.end - f)), dim3(64), lds_ins, s, b);
        ZCHK(hipGetLastError());
      }
      info.slices = std::max(info.slices, slices);
      ZCHK(hipEventRecord(ev[1].e, s));
      // the reverse phase: group the round's requests by (level, target, source), then one wave per (level, target)
      const uint64_t slots = req_off[r.end] - req_off[r.first];
      ZCHK(hipcub::DeviceRadixSort::SortKeys(sort_tmp.p, tmp_bytes, req_a.p, req_b.p, (int)slots, 0, 64, s));
      ZCHK(hipMemsetAsync(ngroups, 0, 4, s));
      hipLaunchKernelGGL(hnsw_groups_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, req_b.p, slots, gstart.p, ngroups.p);
      ZCHK(hipGetLastError());
      hipLaunchKernelGGL(hnsw_reverse_kernel, dim3((uint32_t)std::min<uint64_t>(slots, 4096)), dim3(64), lds_rev, s, b, req_b.p, slots,
                         gstart.p, ngroups.p);
      ZCHK(hipGetLastError());
      ZCHK(hipEventRecord(ev[2].e, s));
      ZCHK(hipEventSynchronize(ev[2].e));
      float ms = 0.f;
      ZCHK(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
      info.insert_ms += ms;
      ZCHK(hipEventElapsedTime(&ms, ev[1].e, ev[2].e));
      info.reverse_ms += ms;
    }
    // a pruned list keeps nothing behind its count
    hipLaunchKernelGGL(hnsw_tidy_kernel, dim3((uint32_t)(((uint64_t)n * q.m0 + 255) / 256)), dim3(256), 0, s, arr.nbr0.p, arr.cnt0.p,
                       (uint64_t)n, q.m0);
    ZCHK(hipGetLastError());
    if (up) {
      hipLaunchKernelGGL(hnsw_tidy_kernel, dim3((uint32_t)(((uint64_t)up_slots * q.m + 255) / 256)), dim3(256), 0, s, arr.nbr_up.p,
                         arr.cnt_up.p, (uint64_t)up_slots, q.m);
      ZCHK(hipGetLastError());
    }
    ZCHK(hipStreamSynchronize(s));
    unsigned long long cnt[3];
    ZCHK(hipMemcpy(cnt, counters, sizeof(cnt), hipMemcpyDeviceToHost));
    info.dists = cnt[0]; info.requests = cnt[1]; info.prunes = cnt[2];
  }
  std::swap(h->arr, arr);                        // the old arrays go with the local
  h->n = n; h->m0 = q.m0; h->m = up ? q.m : 0; h->max_level = up ? max_level : 0; h->n_upper = up ? n_upper : 0;
  h->entry = n ? entry : 0;
  h->loaded = true;
  h->built = true;
  h->binfo = info;
  c->hnsw_count = 0;
  return 0;
}

static int hnsw_build_entry(zvec_hip_hnsw_t h, uint64_t n, const float *rows, bool rows_on_device, const uint64_t *keys,
                            const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::unique_lock<FairSharedMutex> w(h->rw);
  return hnsw_build_locked(h, n, rows, rows_on_device, keys, p, levels);
}

// HnswBuilder::train + build (hnsw_builder.cc): every row goes through HnswAlgorithm::add_node (hnsw_algorithm.cc:31-81)
int zvec_hip_hnsw_build(zvec_hip_hnsw_t h, uint64_t n, const float *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                        const uint32_t *levels) {
  return hnsw_build_entry(h, n, rows, false, keys, p, levels);
}

// the same behind a holder whose rows are in device memory already
int zvec_hip_hnsw_build_dev(zvec_hip_hnsw_t h, uint64_t n, const float *d_rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
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
