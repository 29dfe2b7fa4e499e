// api_entry_sparse_ingest.inc.h — C ABI entry points: a sparse index fed from device memory (zvec_hip_sparse_append_dev /
// _append_dense_dev / _from_dense_dev / _search_dense_dev / _ingest_info; device side: zvk_sparse_ingest.hip.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// Every entry is count -> scan -> (check) -> ONE wait -> write.  The wait reads 16 bytes, the status word and the scan's total:
// an append has to know both before the first byte of the store changes (all or nothing, and the store's room depends on the
// total), a dense search needs its queries' lengths on the host, where zvec_hip_sparse_search_dev cuts query blocks, and the
// converter has to compare the total with its caller's capacity.  What is written after the wait is enqueued on the same stream.

extern "C++" {
namespace {

// The device workspace of one call, in 8-byte words:
//   status | total | acc[nseg + 1] | seg_sum | sums[256 u32] | off[nitems + 1] | cnt[nitems] u32 (dense) | rowcnt[rows] u32
struct IngestWs {
  uint32_t nsl = 1;            // slices of a dense row (CSR: 1, an item is a row)
  uint64_t nitems = 0;
  uint32_t *status = nullptr;  // (status, total and acc[0] are consecutive: one memset)
  uint64_t *total = nullptr, *acc = nullptr, *off = nullptr;
  uint32_t *seg_sum = nullptr, *sums = nullptr, *cnt = nullptr, *rowcnt = nullptr;
};

int ingest_ws(DevBuf &buf, uint64_t nitems, bool dense, uint64_t rows, IngestWs *w) {
  const uint64_t nseg = (nitems + SPARSE_INGEST_SEG - 1) / SPARSE_INGEST_SEG;
  const uint64_t o_acc = 2, o_sum = o_acc + nseg + 1, o_sums = o_sum + 1, o_off = o_sums + SPARSE_INGEST_SEG / INVB_SCAN_CHUNK / 2,
                 o_cnt = o_off + nitems + 1, o_rc = o_cnt + (dense ? (nitems + 1) / 2 : 0), words = o_rc + (rows + 1) / 2;
  ZRET(buf.ensure((size_t)words * 8));
  uint64_t *p = buf.as<uint64_t>();
  w->nitems = nitems;
  w->status = reinterpret_cast<uint32_t *>(p); w->total = p + 1; w->acc = p + o_acc; w->off = p + o_off;
  w->seg_sum = reinterpret_cast<uint32_t *>(p + o_sum); w->sums = reinterpret_cast<uint32_t *>(p + o_sums);
  w->cnt = reinterpret_cast<uint32_t *>(p + o_cnt); w->rowcnt = reinterpret_cast<uint32_t *>(p + o_rc);
  return 0;
}

uint32_t ingest_wave_grid(uint64_t items) {            // a wave per item, the waves stride over the items
  return (uint32_t)std::min<uint64_t>((items + SPARSE_INGEST_THREADS / 64 - 1) / (SPARSE_INGEST_THREADS / 64), 2048);
}

// cnt[nitems] (each clamped to `clamp`) -> w.off[nitems + 1], *w.total = the sum; clears the status word.  Segments of 2^20 items
// go through the 32-bit scan of the inverted build one after the other, each on top of the 64-bit sum of those before it.
int ingest_scan(const uint32_t *cnt, uint32_t clamp, const IngestWs &w, hipStream_t s) {
  ZCHK(hipMemsetAsync(w.status, 0, 24, s));
  for (uint64_t i0 = 0, seg = 0; i0 < w.nitems; i0 += SPARSE_INGEST_SEG, ++seg) {
    const uint64_t m = std::min<uint64_t>(SPARSE_INGEST_SEG, w.nitems - i0);
    ZRET(invb_scan(IngestCounts{cnt + i0, w.off + i0, w.acc + seg, clamp}, m, w.sums, w.seg_sum, s));
    hipLaunchKernelGGL(sparse_ingest_seg_kernel, dim3(1), dim3(64), 0, s, w.acc, (uint32_t)seg, (const uint32_t *)w.seg_sum, w.off + i0 + m,
                       w.total);
    ZCHK(hipGetLastError());
  }
  return 0;
}

// the call's one wait
int ingest_read(const IngestWs &w, uint32_t *status, uint64_t *total, hipStream_t s) {
  uint64_t hdr[2] = {0, 0};
  ZCHK(hipMemcpyAsync(hdr, w.status, sizeof(hdr), hipMemcpyDeviceToHost, s));
  ZCHK(hipStreamSynchronize(s));
  *status = (uint32_t)hdr[0];
  *total = hdr[1];
  return 0;
}

// a dense matrix of values `width` bytes wide, as an entry's arguments (n > 0; rows without columns are never read)
int ingest_dense_args_ok(const void *d_rows, uint32_t dim, uint64_t ld, uint32_t width) {
  if ((!d_rows && dim) || ld < dim || reinterpret_cast<uintptr_t>(d_rows) % width != 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return 0;
}

uint32_t ingest_slices(uint32_t dim) { return std::max<uint32_t>(1, (uint32_t)(((uint64_t)dim + SPARSE_INGEST_SLICE - 1) / SPARSE_INGEST_SLICE)); }

// the workspace of n dense rows, the count pass and the scan; rows != 0: room for the rows' counts as well
int ingest_dense_count(DevBuf &buf, uint32_t width, const void *d_rows, uint64_t n, uint32_t dim, uint64_t ld, uint64_t rows, IngestWs *w,
                       hipStream_t s) {
  w->nsl = ingest_slices(dim);
  ZRET(ingest_ws(buf, n * w->nsl, true, rows, w));
  const uint32_t grid = ingest_wave_grid(w->nitems);
  if (width == 2) hipLaunchKernelGGL((sparse_dense_count_kernel<uint16_t>), dim3(grid), dim3(SPARSE_INGEST_THREADS), 0, s,
                                     static_cast<const uint16_t *>(d_rows), n, dim, ld, w->nsl, w->cnt);
  else hipLaunchKernelGGL((sparse_dense_count_kernel<uint32_t>), dim3(grid), dim3(SPARSE_INGEST_THREADS), 0, s,
                          static_cast<const uint32_t *>(d_rows), n, dim, ld, w->nsl, w->cnt);
  ZCHK(hipGetLastError());
  return ingest_scan(w->cnt, 0xffffffffu, *w, s);
}

// the rows' lengths from the scanned item offsets: counts[n] (nullable); a row above `cap` sets the status word
int ingest_row_counts(const IngestWs &w, uint64_t n, uint32_t cap, uint32_t *d_counts, hipStream_t s) {
  hipLaunchKernelGGL(sparse_ingest_rows_kernel, dim3((uint32_t)((n + SPARSE_INGEST_THREADS - 1) / SPARSE_INGEST_THREADS)),
                     dim3(SPARSE_INGEST_THREADS), 0, s, (const uint64_t *)w.off, w.nsl, n, cap, d_counts, w.status);
  ZCHK(hipGetLastError());
  return 0;
}

int ingest_dense_fill(uint32_t width, const void *d_rows, uint64_t n, uint32_t dim, uint64_t ld, const IngestWs &w, uint32_t *d_idx,
                      void *d_val, hipStream_t s) {
  const uint32_t grid = ingest_wave_grid(w.nitems);
  if (width == 2) hipLaunchKernelGGL((sparse_dense_fill_kernel<uint16_t>), dim3(grid), dim3(SPARSE_INGEST_THREADS), 0, s,
                                     static_cast<const uint16_t *>(d_rows), n, dim, ld, w.nsl, (const uint64_t *)w.off, d_idx,
                                     static_cast<uint16_t *>(d_val));
  else hipLaunchKernelGGL((sparse_dense_fill_kernel<uint32_t>), dim3(grid), dim3(SPARSE_INGEST_THREADS), 0, s,
                          static_cast<const uint32_t *>(d_rows), n, dim, ld, w.nsl, (const uint64_t *)w.off, d_idx,
                          static_cast<uint32_t *>(d_val));
  ZCHK(hipGetLastError());
  return 0;
}

// A validated device append, from the wait on: n rows of `total` pairs, their offsets in ws.off (row r begins at r * ws.nsl).
// Room first (the hole bits, then the store: both can refuse, neither changes a row), then the pairs through `pairs(idx, val)` to
// the store's end, offsets and keys, and the counts last, when the stream has drained.
template <typename F>
int ingest_commit(SparseWrite &w, hipStream_t s, uint64_t n, uint64_t total, const IngestWs &ws, const uint64_t *d_keys, int route,
                  std::chrono::steady_clock::time_point t0, F &&pairs) {
  zvec_hip_sparse_s *h = w.h;
  SparseStore &st = h->st;
  ZRET(w.cover(st.n + n));
  ZRET(st.reserve(st.n + n, st.elems + total, s));
  if (total) ZRET(pairs(st.idx + st.elems, static_cast<char *>(st.val) + st.elems * st.width));
  hipLaunchKernelGGL(sparse_ingest_commit_kernel, dim3((uint32_t)((n + SPARSE_INGEST_THREADS - 1) / SPARSE_INGEST_THREADS)),
                     dim3(SPARSE_INGEST_THREADS), 0, s, (const uint64_t *)ws.off, ws.nsl, n, st.elems, st.n, d_keys, st.row_off, st.keys);
  ZCHK(hipGetLastError());
  ZCHK(hipStreamSynchronize(s));
  if (s != w.s) ZCHK(hipStreamSynchronize(w.s));       // (the hole bits grow on the handle's own stream)
  st.n += n;
  st.elems += total;
  h->ing_route = route;
  h->ing_elems = total;
  const int e = w.finish();
  h->ing_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return e;
}

}  // namespace
}  // extern "C++"

int zvec_hip_sparse_append_dev(zvec_hip_sparse_t h, const uint32_t *d_counts, const uint32_t *d_indices, const void *d_values, uint64_t n,
                               uint64_t elements, const uint64_t *d_keys, void *stream) {
  if (!h || (n && !d_counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (elements && (!d_indices || !d_values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  SparseWrite w(h);
  SparseStore &st = h->st;
  if (st.n + n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (positions are 32-bit in the partial lists)
  ZRET(w.open());
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w.s;
  IngestWs ws;
  ZRET(ingest_ws(h->ing_ws, n, false, 0, &ws));
  ZRET(ingest_scan(d_counts, SPARSE_MAX_COUNT + 1, ws, s));
  hipLaunchKernelGGL(sparse_csr_check_kernel, dim3(ingest_wave_grid(n)), dim3(SPARSE_INGEST_THREADS), 0, s, d_counts, d_indices,
                     (const uint64_t *)ws.off, n, elements, ws.status);
  ZCHK(hipGetLastError());
  uint32_t status = 0;
  uint64_t total = 0;
  ZRET(ingest_read(ws, &status, &total, s));
  if (status || total != elements) return ZVEC_HIP_ERR_INVALID_ARGUMENT;      // (nothing of the store has changed)
  return ingest_commit(w, s, n, total, ws, d_keys, 0, t0, [&](uint32_t *idx, void *val) -> int {
    ZCHK(hipMemcpyAsync(idx, d_indices, (size_t)total * 4, hipMemcpyDeviceToDevice, s));
    ZCHK(hipMemcpyAsync(val, d_values, (size_t)total * st.width, hipMemcpyDeviceToDevice, s));
    return 0;
  });
}

int zvec_hip_sparse_append_dense_dev(zvec_hip_sparse_t h, const void *d_rows, uint64_t n, uint32_t dim, uint64_t ld, const uint64_t *d_keys,
                                     void *stream) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return ld < dim ? ZVEC_HIP_ERR_INVALID_ARGUMENT : 0;
  ZRET(ingest_dense_args_ok(d_rows, dim, ld, h->st.width));      // (the width never changes after create)
  const auto t0 = std::chrono::steady_clock::now();
  SparseWrite w(h);
  SparseStore &st = h->st;
  if (st.n + n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  ZRET(w.open());
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w.s;
  IngestWs ws;
  ZRET(ingest_dense_count(h->ing_ws, st.width, d_rows, n, dim, ld, 0, &ws, s));
  ZRET(ingest_row_counts(ws, n, SPARSE_MAX_COUNT, nullptr, s));
  uint32_t status = 0;
  uint64_t total = 0;
  ZRET(ingest_read(ws, &status, &total, s));
  if (status) return ZVEC_HIP_ERR_INVALID_ARGUMENT;              // (a row above the cap: nothing of the store has changed)
  return ingest_commit(w, s, n, total, ws, d_keys, 1, t0, [&](uint32_t *idx, void *val) -> int {
    return ingest_dense_fill(st.width, d_rows, n, dim, ld, ws, idx, val, s);
  });
}

int zvec_hip_sparse_from_dense_dev(zvec_hip_ctx_t ctx, int dtype, const void *d_in, uint64_t n, uint32_t dim, uint64_t ld, uint32_t *d_counts,
                                   uint32_t *d_indices, void *d_values, uint64_t elems_cap, uint64_t *elements, void *stream) {
  if (elements) *elements = 0;
  if (!ctx || !elements) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype != ZVEC_HIP_DT_FP32 && dtype != ZVEC_HIP_DT_FP16) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (ld < dim) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  const uint32_t width = dtype == ZVEC_HIP_DT_FP16 ? 2u : 4u;
  ZRET(ingest_dense_args_ok(d_in, dim, ld, width));
  if (!d_counts) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ZCHK(hipSetDevice(ctx->device));
  hipStream_t s = pick_stream(ctx, stream);
  IngestWs ws;
  ZRET(ingest_dense_count(ctx->sp_ing, width, d_in, n, dim, ld, 0, &ws, s));
  ZRET(ingest_row_counts(ws, n, 0xffffffffu, d_counts, s));      // (no cap: the converter does not know an index's)
  uint32_t status = 0;
  ZRET(ingest_read(ws, &status, elements, s));
  if (!d_indices || !d_values || *elements == 0) return 0;       // a size query
  if (*elements > elems_cap) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  return ingest_dense_fill(width, d_in, n, dim, ld, ws, d_indices, d_values, s);
}

int zvec_hip_sparse_search_dense_dev(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t dim, uint64_t ld,
                                     uint32_t topk, float threshold, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                                     float *d_out_scores, uint32_t *d_out_counts, void *stream) {
  if (!h || !d_out_keys || !d_out_scores || !d_out_counts || ld < dim) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const uint32_t width = h->st.width;                            // (never changes after create)
  ZRET(ingest_dense_args_ok(d_queries, dim, ld, width));
  if (count > (1u << 19)) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (as zvec_hip_sparse_search_dev)
  if (!merge_fits(topk)) return ZVEC_HIP_ERR_UNSUPPORTED;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = pick_stream(c, stream);
  IngestWs ws;
  ZRET(ingest_dense_count(c->sp_ing, width, d_queries, count, dim, ld, count, &ws, s));
  ZRET(ingest_row_counts(ws, count, SPARSE_MAX_COUNT, ws.rowcnt, s));
  std::vector<uint32_t> q_counts(count);
  ZCHK(hipMemcpyAsync(q_counts.data(), ws.rowcnt, (size_t)count * 4, hipMemcpyDeviceToHost, s));
  uint32_t status = 0;
  uint64_t total = 0;
  ZRET(ingest_read(ws, &status, &total, s));                     // (the lengths have arrived with it)
  if (status) return ZVEC_HIP_ERR_INVALID_ARGUMENT;              // (a query above the cap: no output is touched)
  // indices | values in one block, the values starting at byte te * 4, as the host-pointer entries stage them
  const size_t te = std::max<size_t>((size_t)total, 1);
  ZRET(c->sp_ing_pairs.ensure(te * 4 + te * width));
  uint32_t *d_qidx = c->sp_ing_pairs.as<uint32_t>();
  void *d_qval = d_qidx + te;
  if (total) ZRET(ingest_dense_fill(width, d_queries, count, dim, ld, ws, d_qidx, d_qval, s));
  std::shared_lock<FairSharedMutex> r(h->rw, std::defer_lock);
  ZRET(sparse_lock_current(h, r));
  return sparse_search_locked(h, c, q_counts.data(), d_qidx, d_qval, count, topk, threshold, d_exclude_bitset, d_out_keys, d_out_scores,
                              d_out_counts, s);
}

int zvec_hip_sparse_ingest_info(zvec_hip_sparse_t h, int *route, uint64_t *elements, uint32_t *slice_cols, double *ms) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (route) *route = h->ing_route;
  if (elements) *elements = h->ing_elems;
  if (slice_cols) *slice_cols = SPARSE_INGEST_SLICE;
  if (ms) *ms = h->ing_ms;
  return 0;
}
