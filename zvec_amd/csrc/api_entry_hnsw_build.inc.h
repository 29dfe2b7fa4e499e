// api_entry_hnsw_build.inc.h — C ABI entry points: building an HNSW graph from rows on the device (zvec_hip_hnsw_build*; inside
// extern "C").  Device code: zvk_hnsw_build.hip.h; host planning: host/hnsw_add_plan.h.  Rows in, searchable graph out: the handle of
// api_entry_hnsw.inc.h then answers search, info, export and get_vectors as after a load.  The rule is DESIGN §3c "Building":
// HnswAlgorithm::add_node, update_neighbors and reverse_update_neighbors (hnsw_algorithm.cc:31-81, 394-515) applied in rounds.
// hnsw_plan_call and hnsw_insert_apply are shared with the append (api_entry_hnsw_add.inc.h): plan, then prepare, then mutate.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

static_assert(HNSW_PLAN_MAX_LEVEL == HNSW_BUILD_MAX_LEVEL && HNSW_PLAN_MAX_EF == HNSW_MAX_EF && HNSW_PLAN_MAX_M0 == HNSW_BUILD_MAX_M0 &&
              HNSW_PLAN_MAX_M == HNSW_BUILD_MAX_M && HNSW_PLAN_C_LDS == HNSW_C_LDS, "host/hnsw_add_plan.h restates the kernels' limits");

// HnswAlgorithm::get_random_level (hnsw_algorithm.h) in integer arithmetic
int zvec_hip_hnsw_build_levels(uint64_t n, uint32_t scaling_factor, uint64_t seed, uint32_t *out_levels) {
  return hnsw_levels_range(0, n, scaling_factor, seed, out_levels);
}

struct HnswEvent {
  hipEvent_t e = nullptr;
  ~HnswEvent() { if (e) (void)hipEventDestroy(e); }
};

// What the rounds of one plan need on the device beside the graph; prepare() allocates all of it, so that nothing is refused once
// the graph has changed.  A plan without rounds needs nothing.
struct HnswRoundsScratch {
  Scoped<uint32_t> levels, gstart, ngroups;
  Scoped<uint64_t> req_off, req_a, req_b;
  Scoped<unsigned long long> counters;
  Scoped<unsigned char> sort_tmp;
  size_t tmp_bytes = 0;
  HnswEvent ev[3];
  int prepare(zvec_hip_ctx_s *c, const HnswInsertPlan &pl) {
    if (pl.rounds.empty()) return 0;
    ZRET(upload(levels, pl.lv.data(), pl.lv.size()));
    ZRET(upload(req_off, pl.req_off.data(), pl.req_off.size()));
    ZRET(req_a.alloc(pl.need.max_slots));
    ZRET(counters.alloc(3));
    ZCHK(hipMemset(counters, 0, 3 * sizeof(unsigned long long)));
    if (pl.need.multi) {
      ZRET(req_b.alloc(pl.need.max_slots));
      ZRET(gstart.alloc(pl.need.max_slots));
      ZRET(ngroups.alloc(1));
      ZCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, req_a.p, req_b.p, (int)pl.need.max_slots, 0, 64, c->cur));
      ZRET(sort_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    }
    ZRET(c->hnsw_ws.ensure((size_t)pl.need.max_ws));
    for (HnswEvent &e : ev) ZCHK(hipEventCreate(&e.e));
    return 0;
  }
};

// The rounds of `pl` on the graph g: resized for the plan's shape, the new rows and their upper_of in place, n still the old count.
// A round of one node applies its requests straight from the round buffer (hnsw_reverse_one_kernel); a round of more sorts and groups
// them first.  The caller holds an HnswWrite and has synchronised the device.
static int hnsw_run_rounds(zvec_hip_hnsw_s *h, const HnswGraph &g, const HnswInsertPlan &pl, HnswRoundsScratch &w, HnswInsertDone &done) {
  if (pl.rounds.empty()) return 0;
  zvec_hip_ctx_s *c = h->defctx;
  hipStream_t s = c->cur;
  const zvec_hip_hnsw_build_params &q = pl.q;
  HnswBuildArgs b{};
  HnswArgs &a = b.g;
  a = g.args(h->dim, h->dpad, h->metric);
  a.n = pl.rounds.back().end; a.m = q.m;
  a.ef = q.ef_construction; a.max_scan = 0xffffffffu; a.threshold = 0.f;
  b.nbr0 = g.arr.nbr0; b.cnt0 = g.arr.cnt0; b.nbr_up = g.arr.nbr_up; b.cnt_up = g.arr.cnt_up;
  b.node_base = pl.base; b.levels = w.levels; b.req_off = w.req_off; b.req = w.req_a;
  b.prune_cnt = q.prune_cnt; b.min_neighbors = q.min_neighbors; b.counters = w.counters;
  const size_t lds_ins = hnsw_insert_lds_bytes(a.dpad, a.ef), lds_rev = hnsw_reverse_lds_bytes(a.dpad);
  for (const HnswRound &r : pl.rounds) {
    const bool spill = r.first > HNSW_C_LDS;
    a.entry = r.entry; a.ccap = r.first; a.vis_words = (r.first + 31) / 32;
    b.round_first = r.first; b.top = r.top; b.req_base = pl.req_off[r.first - pl.base];
    const uint32_t slice = hnsw_round_slice(r, pl.budget);
    a.cand_ws = spill ? c->hnsw_ws.as<uint64_t>() : nullptr;
    a.visited = reinterpret_cast<uint32_t *>(c->hnsw_ws.as<uint64_t>() + (spill ? (size_t)slice * a.ccap : 0));
    ZCHK(hipEventRecord(w.ev[0].e, s));
    uint32_t slices = 0;
    for (uint32_t f = r.first; f < r.end; f += slice, ++slices) {     // (the graph is frozen: a slice sees what every slice sees)
      b.first = f;
      hipLaunchKernelGGL(HNSW_KERNEL(h, hnsw_insert_kernel), dim3(std::min(slice, r.end - f)), dim3(64), lds_ins, s, b);
      ZCHK(hipGetLastError());
    }
    done.slices = std::max(done.slices, slices);
    ZCHK(hipEventRecord(w.ev[1].e, s));
    const uint64_t slots = pl.req_off[r.end - pl.base] - pl.req_off[r.first - pl.base];
    if (r.end - r.first == 1) {
      // the reverse phase of one node: every used request word is a (level, target) group of its own
      hipLaunchKernelGGL(HNSW_KERNEL(h, hnsw_reverse_one_kernel), dim3((uint32_t)std::min<uint64_t>(slots, 4096)), dim3(64), lds_rev, s, b, slots);
      ZCHK(hipGetLastError());
      ++done.one;
    } else {
      // the reverse phase: group the round's requests by (level, target, source), then one wave per (level, target)
      ZCHK(hipcub::DeviceRadixSort::SortKeys(w.sort_tmp.p, w.tmp_bytes, w.req_a.p, w.req_b.p, (int)slots, 0, 64, s));
      ZCHK(hipMemsetAsync(w.ngroups, 0, 4, s));
      hipLaunchKernelGGL(hnsw_groups_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, s, w.req_b.p, slots, w.gstart.p, w.ngroups.p);
      ZCHK(hipGetLastError());
      hipLaunchKernelGGL(HNSW_KERNEL(h, hnsw_reverse_kernel), dim3((uint32_t)std::min<uint64_t>(slots, 4096)), dim3(64), lds_rev, s, b,
                         w.req_b.p, slots, w.gstart.p, w.ngroups.p);
      ZCHK(hipGetLastError());
    }
    ZCHK(hipEventRecord(w.ev[2].e, s));
    ZCHK(hipEventSynchronize(w.ev[2].e));
    float ms = 0.f;
    ZCHK(hipEventElapsedTime(&ms, w.ev[0].e, w.ev[1].e));
    done.insert_ms += ms;
    ZCHK(hipEventElapsedTime(&ms, w.ev[1].e, w.ev[2].e));
    done.reverse_ms += ms;
  }
  ZCHK(hipStreamSynchronize(s));
  unsigned long long cnt[3];
  ZCHK(hipMemcpy(cnt, w.counters, sizeof(cnt), hipMemcpyDeviceToHost));
  done.dists = cnt[0]; done.requests = cnt[1]; done.prunes = cnt[2];
  return 0;
}

// What both entries hand hnsw_insert_plan beside their own arguments: the two round options and the workspace budget.
static int hnsw_plan_call(const HnswShape &found, const zvec_hip_hnsw_s *h, bool append, uint64_t count, const void *rows,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels, HnswInsertPlan &pl) {
  const zvec_hip_hnsw_build_params none{};
  return hnsw_insert_plan(found, append ? h->params : none, append ? h->want_rows : 0, append ? h->want_upper : 0, count, rows != nullptr, p,
                          levels, (uint32_t)ropts().hnsw_build_round_div.load(std::memory_order_relaxed),
                          (uint32_t)ropts().hnsw_build_round_max.load(std::memory_order_relaxed),
                          (uint64_t)ropts().hnsw_ws_bytes.load(std::memory_order_relaxed), append, pl);
}

// Carries a plan out on g, the handle's graph or a fresh one: prepare, then mutate.  Everything that can be refused for want of
// memory is allocated first, the rounds' scratch (1) and the larger arrays (2, whose new blocks exist before g takes them); from the
// first write to g on (the swap at the end of HnswGraph::resize) only a HIP copy, launch or synchronise can fail.  So a call refused
// for memory leaves g as it found it, possibly with more room.  rows: [pl.count][dim], on the device or on the host.  The caller
// holds an HnswWrite and has synchronised the device.
static int hnsw_insert_apply(zvec_hip_hnsw_s *h, HnswGraph &g, const HnswInsertPlan &pl, const void *rows, bool rows_on_device,
                             const uint64_t *keys, HnswInsertDone &done) {
  done = HnswInsertDone();
  HnswRoundsScratch w;
  ZRET(w.prepare(h->defctx, pl));                                                                  // 1
  ZRET(g.resize(pl.after, h->pad_bytes(), h->defctx->cur, done.grew_rows, done.grew_upper));       // 2
  ZRET(g.put_rows(pl.base, pl.count, rows, rows_on_device, keys, h->row_bytes(), h->pad_bytes())); // 3: behind the old rows; their lists
  if (pl.after.stride)                                                                             //    and counts are zero already
    ZCHK(hipMemcpy(g.arr.upper_of.p + pl.base, pl.upper_of.data(), (size_t)pl.count * 4, hipMemcpyHostToDevice));
  ZCHK(hipDeviceSynchronize());                  // (a device-to-device copy of rows may still be in flight on the null stream)
  ZRET(hnsw_run_rounds(h, g, pl, w, done));                                                        // 4
  static_cast<HnswShape &>(g) = pl.after;                                                          // 5
  done.rounds = (uint32_t)pl.rounds.size(); done.top = pl.top; done.entry = pl.after.entry;
  done.first = pl.base; done.count = pl.count; done.restrided = pl.restride;
  done.cap_rows = g.cap_rows; done.cap_upper = g.cap_upper;
  return 0;
}

// the fields zvec_hip_hnsw_build_info and zvec_hip_hnsw_add_info share
extern "C++" template <typename Info>
static void hnsw_info_common(Info &out, const HnswInsertDone &d) {
  out.rounds = d.rounds; out.slices = d.slices; out.top = d.top; out.entry_point = d.entry;
  out.dists = d.dists; out.requests = d.requests; out.prunes = d.prunes;
  out.insert_ms = d.insert_ms; out.reverse_ms = d.reverse_ms;
}

// A build is an insertion from base 0 into a fresh graph that takes the old one's place on success: it finds no graph, remembers
// nothing and asks for no room beyond its rows, whatever a reserve said.
static int hnsw_build_entry(zvec_hip_hnsw_t h, uint64_t n, const void *rows, bool rows_on_device, const uint64_t *keys,
                            const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  HnswWrite w(h);
  ZRET(w.open());
  HnswInsertPlan pl;
  ZRET(hnsw_plan_call(HnswShape(), h, false, n, rows, p, levels, pl));
  ZRET(w.quiesce());
  HnswGraph g;
  HnswInsertDone done;
  ZRET(hnsw_insert_apply(h, g, pl, rows, rows_on_device, keys, done));
  hnsw_commit(h, g);                             // the old arrays go with the local
  h->params = pl.q;
  h->built = true;
  h->bdone = done;
  return 0;
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
  *out = zvec_hip_hnsw_build_info();
  hnsw_info_common(*out, h->bdone);
  return 0;
}
