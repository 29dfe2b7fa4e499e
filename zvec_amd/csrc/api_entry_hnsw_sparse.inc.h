// api_entry_hnsw_sparse.inc.h — C ABI entry points: batched k-NN search on a built HNSW graph over SPARSE rows
// (zvec_hip_hnsw_sparse_*; inside extern "C").  Device code: zvk_hnsw_sparse.hip.h.  The twin of api_entry_hnsw.inc.h for
// HnswSparseSearcher (src/core/algorithm/hnsw_sparse/hnsw_sparse_searcher.cc): the graph arrays, their validation, the sliced search,
// the statistics and the write scope are that file's (HnswGraph, hnsw_validate, hnsw_search_sliced, hnsw_last_stats_of,
// HnswWriteOf); the rows are CSR as the sparse flat store keeps them, and the run checks and the query staging are
// api_entry_sparse.inc.h's.  Loads a graph somebody else built; api_entry_hnsw_sparse_build.inc.h builds one.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

struct zvec_hip_hnsw_sparse_s {
  int device = 0;
  int dtype = ZVEC_HIP_DT_FP32;        // of the values of rows and queries; halves are stored as halves
  uint32_t width = 4;                  // bytes per value
  bool loaded = false;
  HnswGraph graph;                     // keys and lists; graph.arr.rows stays empty, the rows are the three arrays below
  Scoped<uint64_t> row_off;            // [n + 1]
  Scoped<uint32_t> idx;                // [elems]
  Scoped<unsigned char> val;           // [elems] values of `width` bytes
  uint64_t elems = 0;
  zvec_hip_hnsw_build_params params{};           // of the last build; all zero after a load
  bool built = false;                  // bdone is the last build's
  HnswInsertDone bdone;
  zvec_hip_ctx_s *defctx = nullptr;
  std::mutex mu;                       // lock order and meaning as zvec_hip_hnsw_s
  FairSharedMutex rw;
  ~zvec_hip_hnsw_sparse_s() { delete defctx; }
};

// The rows of a graph in fresh blocks of their own, CSR as the sparse flat store keeps them: what a load or a build makes whole
// before the handle changes.  counts [n] on the host (total = their sum); the pairs on the host, or on the device.
struct HnswSparseRows {
  Scoped<uint64_t> row_off;
  Scoped<uint32_t> idx;
  Scoped<unsigned char> val;
  uint64_t elems = 0;
  int put(const uint32_t *counts, uint64_t n, uint64_t total, const uint32_t *indices, const void *values, uint32_t width, bool on_device) {
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + counts[i];
    ZRET(upload(row_off, off.data(), off.size()));
    ZRET(idx.alloc(std::max<size_t>(total, 1)));
    ZRET(val.alloc(std::max<size_t>(total, 1) * width));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (total) {
      ZCHK(hipMemcpy(idx.p, indices, (size_t)total * 4, kind));
      ZCHK(hipMemcpy(val.p, values, (size_t)total * width, kind));
    }
    elems = total;
    return 0;
  }
};

// The one place a graph and its rows become the handle's (hnsw_commit's twin); the old arrays go with g and rows.
static void hnsw_sparse_commit(zvec_hip_hnsw_sparse_s *h, HnswGraph &g, HnswSparseRows &rows) {
  std::swap(h->graph, g);
  static_cast<HnswShape &>(h->graph) = hnsw_shape_kept(h->graph);
  std::swap(h->row_off, rows.row_off); std::swap(h->idx, rows.idx); std::swap(h->val, rows.val);
  h->elems = rows.elems;
  h->loaded = true;
  h->defctx->last.begin(LastSearch::NONE, nullptr);       // (the statistics of a search of the graph that went)
}

int zvec_hip_hnsw_sparse_create(int dtype, int metric, int device, zvec_hip_hnsw_sparse_t *out) {
  if (!out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype != ZVEC_HIP_DT_FP32 && dtype != ZVEC_HIP_DT_FP16) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (metric != ZVEC_HIP_METRIC_IP) return ZVEC_HIP_ERR_UNSUPPORTED;       // (SquaredEuclideanSparse is not served)
  zvec_hip_ctx_s *c = nullptr;
  ZRET(ctx_new(device, &c));
  zvec_hip_hnsw_sparse_s *h = new (std::nothrow) zvec_hip_hnsw_sparse_s();
  if (!h) { ctx_free(c); return ZVEC_HIP_ERR_NO_MEMORY; }
  h->device = device; h->dtype = dtype; h->width = dtype == ZVEC_HIP_DT_FP16 ? 2u : 4u; h->defctx = c;
  *out = h;
  return 0;
}

int zvec_hip_hnsw_sparse_dtype(zvec_hip_hnsw_sparse_t h, int *dtype) {
  if (!h || !dtype) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  *dtype = h->dtype;
  return 0;
}

int zvec_hip_hnsw_sparse_destroy(zvec_hip_hnsw_sparse_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
  return 0;
}

// HnswSparseSearcher::load in the shape of plain arrays: the rows as zvec_hip_sparse_append takes them, the graph as zvec_hip_hnsw_load
int zvec_hip_hnsw_sparse_load(zvec_hip_hnsw_sparse_t h, uint64_t n, const uint32_t *counts, const uint32_t *indices, const void *values,
                              const uint64_t *keys, uint32_t m0, const uint32_t *nbr0, const uint32_t *cnt0, uint32_t max_level, uint32_t m,
                              uint32_t n_upper, const uint32_t *upper_of, const uint32_t *nbr_up, const uint32_t *cnt_up,
                              uint32_t entry_point) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZRET(hnsw_validate(n, counts, m0, nbr0, cnt0, max_level, m, n_upper, upper_of, nbr_up, cnt_up, entry_point));
  uint64_t total = 0;
  if (n) ZRET(sparse_check_runs(counts, indices, n, &total));
  if (total && (!indices || !values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  HnswWriteOf<zvec_hip_hnsw_sparse_s> w(h);
  ZRET(w.open());
  ZRET(w.quiesce());
  HnswGraph g;                                   // everything new is whole before the handle changes
  HnswShape to;
  to.n = to.cap_rows = n; to.m0 = m0; to.m = m; to.stride = max_level; to.n_upper = n_upper; to.cap_upper = n_upper; to.entry = entry_point;
  ZRET(g.load_lists(to, 0, h->defctx->cur, nbr0, cnt0, upper_of, nbr_up, cnt_up));
  ZRET(g.put_keys(0, n, keys));
  HnswSparseRows rows;
  ZRET(rows.put(counts, n, total, indices, values, h->width, false));
  hnsw_sparse_commit(h, g, rows);                // the old arrays go with the locals
  h->params = zvec_hip_hnsw_build_params();
  return 0;
}

int zvec_hip_hnsw_sparse_info(zvec_hip_hnsw_sparse_t h, uint64_t *n, uint64_t *elements, uint32_t *m0, uint32_t *max_level, uint32_t *m,
                              uint32_t *n_upper, uint32_t *entry_point) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  const HnswShape &g = h->graph;
  if (n) *n = g.n;
  if (elements) *elements = h->elems;
  if (m0) *m0 = g.m0;
  if (max_level) *max_level = g.stride;
  if (m) *m = g.m;
  if (n_upper) *n_upper = g.n_upper;
  if (entry_point) *entry_point = g.entry;
  return 0;
}

// HnswSparseEntity::get_vector: the row at `position` as it is stored
int zvec_hip_hnsw_sparse_get_vector(zvec_hip_hnsw_sparse_t h, uint64_t position, uint32_t *count, uint32_t *indices, void *values) {
  if (!h || !count) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (position >= h->graph.n) return ZVEC_HIP_ERR_NO_EXIST;
  ZCHK(hipSetDevice(h->device));
  uint64_t be[2];
  ZCHK(hipMemcpy(be, h->row_off.p + position, 16, hipMemcpyDeviceToHost));
  const size_t c = (size_t)(be[1] - be[0]);
  *count = (uint32_t)c;
  if (c && indices) ZCHK(hipMemcpy(indices, h->idx.p + be[0], c * 4, hipMemcpyDeviceToHost));
  if (c && values) ZCHK(hipMemcpy(values, h->val.p + be[0] * h->width, c * h->width, hipMemcpyDeviceToHost));
  return 0;
}

int zvec_hip_hnsw_sparse_export(zvec_hip_hnsw_sparse_t h, uint64_t *keys, uint32_t *nbr0, uint32_t *cnt0, uint32_t *upper_of,
                                uint32_t *nbr_up, uint32_t *cnt_up) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (h->graph.n == 0) return 0;
  ZCHK(hipSetDevice(h->device));
  return h->graph.export_lists(keys, nbr0, cnt0, upper_of, nbr_up, cnt_up);
}

// The search proper; the caller holds c->mu and h->rw (shared); q_counts (HOST) has passed sparse_check_runs, everything else is on
// the device.  The element offsets of the queries go up through the context's plan slot (sparse_upload_plan), the walk in the slices
// of hnsw_search_sliced.
static int hnsw_sparse_search_dev_locked(zvec_hip_hnsw_sparse_s *h, zvec_hip_ctx_s *c, const uint32_t *q_counts, const uint32_t *d_qidx,
                                         const void *d_qval, uint32_t count, uint32_t topk, uint32_t ef, uint32_t max_scan,
                                         float threshold, const uint64_t *d_exclude, uint64_t *d_out_keys, float *d_out_scores,
                                         uint32_t *d_out_counts, hipStream_t s) {
  HnswSparseArgs sa{};
  if (h->graph.n) {
    std::vector<uint32_t> plan((size_t)count + 1, 0u);
    uint32_t max_run = 0;
    for (uint32_t q = 0; q < count; ++q) {
      plan[q + 1] = plan[q] + q_counts[q];
      max_run = std::max(max_run, q_counts[q]);
    }
    // (never truncated: a walk whose run, R and C do not fit is refused whole)
    if (hnsw_search_lds_bytes(hnsw_sparse_run_bytes(max_run, h->width), std::max(ef, topk), HnswCsrRows<float>::SCRATCH) > HNSW_LDS_UNRAISED)
      return ZVEC_HIP_ERR_UNSUPPORTED;
    ZRET(sparse_upload_plan(c, plan, s));
    sa.op = SparseOperands{h->row_off, h->idx, h->val, nullptr, c->sp_plan.as<uint32_t>(), d_qidx, d_qval};
    sa.run_bytes = (uint32_t)hnsw_sparse_run_bytes(max_run, h->width);
  }
  const size_t run_bytes = sa.run_bytes;
  return hnsw_search_sliced(h, h->graph, h->graph.args(0, 0, ZVEC_HIP_METRIC_IP), c, count, topk, ef, max_scan, threshold, d_exclude,
                            d_out_keys, d_out_scores, d_out_counts, s, [&](HnswArgs &a, uint32_t q0, uint32_t mq) -> int {
    sa.g = a;
    sa.q0 = q0;
    const size_t lds = hnsw_search_lds_bytes(run_bytes, a.ef, HnswCsrRows<float>::SCRATCH);
    if (h->width == 2) hipLaunchKernelGGL(hnsw_sparse_search_kernel<_Float16>, dim3(mq), dim3(64), lds, s, sa);
    else hipLaunchKernelGGL(hnsw_sparse_search_kernel<float>, dim3(mq), dim3(64), lds, s, sa);
    ZCHK(hipGetLastError());
    return 0;
  });
}

// the arguments of both search entries, in the order the codes are documented: pointers, count == 0 (the caller returns), topk, the
// list length, then the runs as zvec_hip_sparse_search judges them
static int hnsw_sparse_search_args(const void *h, const uint32_t *q_counts, uint32_t count, uint32_t topk, uint32_t ef, const void *keys,
                                   const void *scores, const void *counts) {
  if (!h || !keys || !scores || !counts || (count && !q_counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count && topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return std::max(ef, topk) > HNSW_MAX_EF ? ZVEC_HIP_ERR_UNSUPPORTED : 0;
}

// HnswSparseSearcher::search_impl (hnsw_sparse_searcher.cc) above the brute-force hand-over, which stays with the caller
int zvec_hip_hnsw_sparse_search_dev(zvec_hip_hnsw_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *d_q_indices,
                                    const void *d_q_values, uint32_t count, uint32_t topk, uint32_t ef, uint32_t max_scan, float threshold,
                                    const uint64_t *d_exclude_bitset, uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts,
                                    void *stream) {
  ZRET(hnsw_sparse_search_args(h, q_counts, count, topk, ef, d_out_keys, d_out_scores, d_out_counts));
  if (count == 0) return 0;
  if (count > (1u << 19)) return ZVEC_HIP_ERR_OUT_OF_RANGE;          // (query offsets are 32-bit, as zvec_hip_sparse_search_dev)
  uint64_t total = 0;
  ZRET(sparse_check_runs(q_counts, nullptr, count, &total));
  if (total && (!d_q_indices || !d_q_values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  ZCHK(hipSetDevice(h->device));
  return hnsw_sparse_search_dev_locked(h, c, q_counts, d_q_indices, d_q_values, count, topk, ef, max_scan, threshold, d_exclude_bitset,
                                       d_out_keys, d_out_scores, d_out_counts, pick_stream(c, stream));
}

int zvec_hip_hnsw_sparse_search(zvec_hip_hnsw_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                                const void *q_values, uint32_t count, uint32_t topk, uint32_t ef, uint32_t max_scan, float threshold,
                                const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores, uint32_t *out_counts) {
  ZRET(hnsw_sparse_search_args(h, q_counts, count, topk, ef, out_keys, out_scores, out_counts));
  if (count == 0) return 0;
  uint64_t total = 0;
  ZRET(sparse_queries_ok(q_counts, q_indices, q_values, count, 0, &total));
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->width, total, q_indices, q_values, blob, &te);      // (the width never changes after create)
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);                // ONE critical section from the upload to the copy-out (zvec_hip_hnsw_search)
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw);        // the row count the bitset is sized for == the nodes of the graph
    if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
    const bool ex = exclude_bitset && h->graph.n;
    ZRET(host_search_wrap_begin(c, blob.data(), blob.size() * 4, ex ? exclude_bitset : nullptr, h->graph.n, count, topk, c->cur));
    const uint32_t *dq = static_cast<const uint32_t *>(c->io_qp);
    ZRET(hnsw_sparse_search_dev_locked(h, c, q_counts, dq, dq + te, count, topk, ef, max_scan, threshold,
                                       ex ? c->io_ex.as<uint64_t>() : nullptr, c->io_keys.as<uint64_t>(), c->io_scores.as<float>(),
                                       c->io_counts.as<uint32_t>(), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

int zvec_hip_hnsw_sparse_last_stats(zvec_hip_hnsw_sparse_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t *out_scanned, uint32_t *out_hops,
                                    uint32_t *out_slices) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return hnsw_last_stats_of(h, h->device, ctx ? ctx : h->defctx, count, out_scanned, out_hops, out_slices);
}
