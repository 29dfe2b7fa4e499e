// api_entry_hnsw_add.inc.h — C ABI entry points: appending rows to an HNSW graph on the device (zvec_hip_hnsw_add*, _reserve,
// _last_add_info; inside extern "C").  Stands behind HnswStreamer::add_impl / add_with_id_impl (hnsw_streamer.cc:426-585).  The rule
// is DESIGN §3c "Appending": the build's rounds (hnsw_run_rounds, api_entry_hnsw_build.inc.h) started at s = the nodes already
// there, on arrays that grow; host planning: host/hnsw_add_plan.h; device code: zvk_hnsw_build.hip.h.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// dst: a block of new_count elements whose first old_count are src's (device to device) and whose others are `fill` bytes; the work
// is queued on `s`, in order with the kernels that follow on it
extern "C++" template <typename T>
static int hnsw_regrow(Scoped<T> &dst, const Scoped<T> &src, size_t old_count, size_t new_count, int fill, hipStream_t s) {
  ZRET(dst.alloc(std::max<size_t>(new_count, 1)));
  if (old_count) ZCHK(hipMemcpyAsync(dst.p, src.p, old_count * sizeof(T), hipMemcpyDeviceToDevice, s));
  if (new_count > old_count) ZCHK(hipMemsetAsync(dst.p + old_count, fill, (new_count - old_count) * sizeof(T), s));
  return 0;
}

// Gives the handle's arrays room for cap_rows rows and, under the stride `stride` (0: no upper lists, nothing is made), cap_upper
// nodes of level >= 1; m0 / m: the widths of the lists.  Never shrinks; what is not too small stays where it is.  Old slot (u, l)
// of the upper table goes to new slot (u, l); everything behind the old content is zero, upper_of IDX_NONE.  Every new block is
// allocated before the handle changes.  The caller holds the handle exclusively and has synchronised the device.
static int hnsw_resize(zvec_hip_hnsw_s *h, uint64_t cap_rows, uint64_t cap_upper, uint32_t stride, uint32_t m0, uint32_t m, bool &grew_rows,
                       bool &grew_upper) {
  const size_t n = (size_t)h->n, old_stride = h->max_level, old_upper = h->n_upper;
  cap_rows = std::max(cap_rows, h->cap_rows);
  cap_upper = stride ? std::max(cap_upper, h->cap_upper) : 0;
  grew_rows = cap_rows > h->cap_rows;
  const bool make_upper_of = stride && !old_stride;
  const bool move_table = stride && (stride != old_stride || cap_upper > h->cap_upper);
  grew_upper = stride && cap_upper > h->cap_upper;
  zvec_hip_hnsw_s::Arrays g;
  hipStream_t s = h->defctx->cur;
  if (grew_rows) {
    ZRET(hnsw_regrow(g.rows, h->arr.rows, n * h->pad_bytes(), (size_t)cap_rows * h->pad_bytes(), 0, s));
    ZRET(hnsw_regrow(g.keys, h->arr.keys, n, (size_t)cap_rows, 0, s));
    ZRET(hnsw_regrow(g.cnt0, h->arr.cnt0, n, (size_t)cap_rows, 0, s));
    ZRET(hnsw_regrow(g.nbr0, h->arr.nbr0, n * m0, (size_t)cap_rows * m0, 0, s));
  }
  if (stride && (grew_rows || make_upper_of)) ZRET(hnsw_regrow(g.upper_of, h->arr.upper_of, old_stride ? n : 0, (size_t)cap_rows, 0xff, s));
  if (move_table) {
    const size_t slots = (size_t)cap_upper * stride;
    const bool same = stride == old_stride;
    ZRET(hnsw_regrow(g.cnt_up, h->arr.cnt_up, same ? old_upper * old_stride : 0, slots, 0, s));
    ZRET(hnsw_regrow(g.nbr_up, h->arr.nbr_up, same ? old_upper * old_stride * m : 0, slots * m, 0, s));
    if (!same && old_stride && old_upper) {
      const uint64_t threads = (uint64_t)old_upper * old_stride * std::max(m, 1u);
      hipLaunchKernelGGL(hnsw_restride_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, h->arr.nbr_up.p,
                         h->arr.cnt_up.p, g.nbr_up.p, g.cnt_up.p, (uint64_t)old_upper, (uint32_t)old_stride, stride, m);
      ZCHK(hipGetLastError());
    }
  }
  ZCHK(hipStreamSynchronize(s));                 // (the copies have read the old blocks, the new ones are whole)
  if (g.rows.p) { std::swap(h->arr.rows, g.rows); std::swap(h->arr.keys, g.keys); std::swap(h->arr.cnt0, g.cnt0); std::swap(h->arr.nbr0, g.nbr0); }
  if (g.upper_of.p) std::swap(h->arr.upper_of, g.upper_of);
  if (g.cnt_up.p) { std::swap(h->arr.cnt_up, g.cnt_up); std::swap(h->arr.nbr_up, g.nbr_up); }
  h->cap_rows = cap_rows;                        // the old blocks go with the local
  if (stride) { h->cap_upper = cap_upper; h->max_level = stride; h->m = m; }
  return 0;
}

// the caller holds h->mu, the default context's mutex and h->rw exclusively; rows: [count][dim], on the device or on the host
static int hnsw_add_locked(zvec_hip_hnsw_s *h, uint64_t count64, const void *rows, bool rows_on_device, const uint64_t *keys,
                           const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  const bool has = h->loaded && h->n > 0;        // without a graph the call is a build of these rows
  const uint64_t n = has ? h->n : 0;
  zvec_hip_hnsw_build_params q{};
  ZRET(hnsw_add_params(p, h->params, n, has ? h->m0 : 0, has ? h->m : 0, q));
  if (h->dim > HNSW_MAX_DIM || q.m0 == 0) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (count64 && !rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count64 == 0) return 0;                    // (nothing to insert, nothing changes)
  std::vector<uint32_t> lv;
  ZRET(hnsw_add_levels(n, count64, levels, q, lv));
  const uint32_t count = (uint32_t)count64, base = (uint32_t)n;
  const uint32_t round_div = (uint32_t)ropts().hnsw_build_round_div.load(std::memory_order_relaxed);
  const uint32_t round_max = (uint32_t)ropts().hnsw_build_round_max.load(std::memory_order_relaxed);
  std::vector<HnswRound> plan;
  std::vector<uint64_t> req_off;
  uint32_t entry = has ? h->entry : 0, top = has ? h->max_level : 0;      // (the entry point of a graph is on its largest level)
  hnsw_plan_rounds(base, lv.data(), count, round_div, round_max, q.m0, q.m, entry, top, plan, req_off);
  std::vector<uint32_t> upper_of(count);
  const HnswAddShape shape = hnsw_add_shape(has ? h->max_level : 0, has ? h->n_upper : 0, lv.data(), count, upper_of.data());
  const uint64_t budget = (uint64_t)ropts().hnsw_ws_bytes.load(std::memory_order_relaxed);
  const HnswRoundsNeed need = hnsw_rounds_need(plan, req_off, base, budget);
  if (need.max_slots >= (1ull << 31)) return ZVEC_HIP_ERR_UNSUPPORTED;     // (group starts are 32-bit, the sort counts in int)

  zvec_hip_ctx_s *c = h->defctx;
  ZCHK(hipDeviceSynchronize());                  // (searches enqueued on other contexts have finished with the arrays)
  if (!has) {                                    // whatever an empty load or build left: the arrays start from nothing
    zvec_hip_hnsw_s::Arrays none;
    std::swap(h->arr, none);
    h->n = 0; h->m0 = h->m = h->max_level = h->n_upper = h->entry = 0;
    h->cap_rows = h->cap_upper = 0;
  }
  bool grew_rows = false, grew_upper = false;
  ZRET(hnsw_resize(h, hnsw_grow(h->cap_rows, n + count, h->want_rows), shape.stride ? hnsw_grow(h->cap_upper, shape.n_upper, h->want_upper) : 0,
                   shape.stride, q.m0, q.m, grew_rows, grew_upper));
  // the new rows behind the old ones; their lists and counts are zero already
  ZCHK(hipMemcpy2D(h->arr.rows.p + (size_t)n * h->pad_bytes(), h->pad_bytes(), rows, h->row_bytes(), h->row_bytes(), count,
                   rows_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (keys) {
    ZCHK(hipMemcpy(h->arr.keys.p + n, keys, (size_t)count * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<uint64_t> id(count);
    for (uint32_t i = 0; i < count; ++i) id[i] = n + i;
    ZCHK(hipMemcpy(h->arr.keys.p + n, id.data(), (size_t)count * 8, hipMemcpyHostToDevice));
  }
  if (shape.stride) ZCHK(hipMemcpy(h->arr.upper_of.p + n, upper_of.data(), (size_t)count * 4, hipMemcpyHostToDevice));
  ZCHK(hipDeviceSynchronize());                  // (a device-to-device copy of rows may still be in flight on the null stream)
  HnswRoundsDone done;
  ZRET(hnsw_run_rounds(h, h->arr, shape.stride, q, base, lv, plan, req_off, need, budget, done));

  h->n = n + count; h->m0 = q.m0; h->n_upper = shape.n_upper; h->entry = entry;
  if (!has) h->params = q;
  h->loaded = true;
  zvec_hip_hnsw_add_info &info = h->ainfo;
  info = zvec_hip_hnsw_add_info();
  info.rounds = (uint32_t)plan.size(); info.slices = done.slices; info.top = top; info.entry_point = entry;
  info.dists = done.dists; info.requests = done.requests; info.prunes = done.prunes;
  info.insert_ms = done.insert_ms; info.reverse_ms = done.reverse_ms;
  info.first = n; info.count = count; info.rounds_one = done.one;
  info.grew_rows = grew_rows; info.grew_upper = grew_upper; info.restrided = shape.restride;
  info.cap_rows = h->cap_rows; info.cap_upper = h->cap_upper;
  h->added = true;
  c->hnsw_count = 0;
  return 0;
}

static int hnsw_add_entry(zvec_hip_hnsw_t h, uint64_t count, const void *rows, bool rows_on_device, const uint64_t *keys,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::unique_lock<FairSharedMutex> w(h->rw);
  return hnsw_add_locked(h, count, rows, rows_on_device, keys, p, levels);
}

// HnswStreamer::add_impl (hnsw_streamer.cc:426-503) for count rows: each ends in HnswAlgorithm::add_node(id, level, ctx)
int zvec_hip_hnsw_add(zvec_hip_hnsw_t h, uint64_t count, const void *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                      const uint32_t *levels) {
  return hnsw_add_entry(h, count, rows, false, keys, p, levels);
}

// the same behind a holder whose rows are in device memory already
int zvec_hip_hnsw_add_dev(zvec_hip_hnsw_t h, uint64_t count, const void *d_rows, const uint64_t *keys,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  return hnsw_add_entry(h, count, d_rows, true, keys, p, levels);
}

// HnswStreamerEntity grows its storage chunk by chunk (hnsw_streamer_entity.cc); here the room is taken in one step
int zvec_hip_hnsw_reserve(zvec_hip_hnsw_t h, uint64_t rows, uint64_t upper_nodes) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (rows >= HNSW_PLAN_MAX_NODES || upper_nodes >= HNSW_PLAN_MAX_NODES) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  ZCHK(hipSetDevice(h->device));
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::unique_lock<FairSharedMutex> w(h->rw);
  const bool has = h->loaded && h->n > 0;
  const uint32_t sf = h->params.scaling_factor ? h->params.scaling_factor : has && h->m ? h->m : 50;
  const uint64_t upper = upper_nodes ? upper_nodes : hnsw_reserve_upper(rows, sf);
  if (has && (rows > h->cap_rows || (h->max_level && upper > h->cap_upper))) {
    ZCHK(hipDeviceSynchronize());                // (searches enqueued on other contexts have finished with the arrays)
    bool grew_rows, grew_upper;
    ZRET(hnsw_resize(h, rows, upper, h->max_level, h->m0, h->m, grew_rows, grew_upper));
  }
  h->want_rows = std::max(h->want_rows, rows);
  h->want_upper = std::max(h->want_upper, upper);
  return 0;
}

// what the last add of `h` did
int zvec_hip_hnsw_last_add_info(zvec_hip_hnsw_t h, zvec_hip_hnsw_add_info *out) {
  if (!h || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->added) return ZVEC_HIP_ERR_NO_READY;
  *out = h->ainfo;
  return 0;
}
