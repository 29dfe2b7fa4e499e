// api_entry_hamming_ivf_fp32.inc.h — C ABI entry points: the fp32 side of a Hamming IVF handle (inside extern "C").  fp32 rows kept
// beside the lists in list order, a build that encodes them on the device, and a search that takes fp32 queries, runs the Hamming
// chain of api_entry_hamming_ivf.inc.h for the candidates and re-ranks them on the rows without leaving the device.
// Device code: zvk_hamming_rerank.hip.h.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// the handle / dim / metric pairing of every fp32 entry (the converter only emits DT_BINARY32 rows of 32 * ceil(dim / 32) bits)
static int bivf_fp32_pairs(const zvec_hip_bivf_s *h, uint32_t dim, int metric) {
  if (!benc_args_ok(dim, dim)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (h->dtype != ZVEC_HIP_DT_BINARY32 || h->lists.dim_in != benc_words(dim) * 32u) return ZVEC_HIP_ERR_MISMATCH;
  return metric == ZVEC_HIP_METRIC_L2 || metric == ZVEC_HIP_METRIC_IP ? 0 : ZVEC_HIP_ERR_UNSUPPORTED;
}

static int launch_gather_f32_rows(const float *d_src, const uint64_t *d_perm, uint64_t n, uint32_t dim, float *d_dst, hipStream_t s) {
  hipLaunchKernelGGL(bivf_gather_f32_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, d_src, d_perm, n, dim, d_dst);
  ZCHK(hipGetLastError());
  return 0;
}

// fp32 DEVICE rows -> sign bits -> the build -> the rows gathered into list order.  Everything the fp32 side needs is allocated
// before the index is touched.  The caller holds the write scope.
static int bivf_build_fp32_locked(BivfWrite &w, const float *d_rows, uint64_t n, uint32_t dim, int metric, const uint64_t *keys,
                                  uint32_t nlist, uint32_t iters, uint64_t seed, float bin_threshold, hipStream_t s) {
  zvec_hip_bivf_s *h = w.h;
  Scoped<float> fresh;
  Scoped<uint32_t> d_bits;
  Scoped<uint64_t> d_perm;
  ZRET(fresh.alloc((size_t)n * dim));
  ZRET(d_bits.alloc((size_t)n * benc_words(dim)));
  ZRET(launch_binary_encode(d_rows, n, dim, dim, bin_threshold, d_bits, s));
  ZRET(bivf_build_locked(w, d_bits, n, keys, nlist, iters, seed, s, &d_perm));
  ZRET(launch_gather_f32_rows(d_rows, d_perm, n, dim, fresh, s));
  ZCHK(hipStreamSynchronize(s));           // (d_perm and d_bits are locals)
  h->frows = std::move(fresh);
  h->fdim = dim;
  h->fmetric = metric;
  return 0;
}

int zvec_hip_bivf_build_fp32_dev(zvec_hip_bivf_t h, const float *d_rows, uint64_t n, uint32_t dim, int metric, const uint64_t *keys,
                                 uint32_t nlist, uint32_t kmeans_iters, uint64_t seed, float bin_threshold, void *stream) {
  ZRET(bivf_build_args(h, d_rows, n, nlist));
  ZRET(bivf_fp32_pairs(h, dim, metric));
  ZCHK(hipSetDevice(h->device));
  BivfWrite w(h);
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : h->defctx->own;
  return w.done(bivf_build_fp32_locked(w, d_rows, n, dim, metric, keys, nlist, kmeans_iters, seed, bin_threshold, s), s);
}

int zvec_hip_bivf_build_fp32(zvec_hip_bivf_t h, const float *rows, uint64_t n, uint32_t dim, int metric, const uint64_t *keys, uint32_t nlist,
                             uint32_t kmeans_iters, uint64_t seed, float bin_threshold) {
  ZRET(bivf_build_args(h, rows, n, nlist));
  ZRET(bivf_fp32_pairs(h, dim, metric));
  ZCHK(hipSetDevice(h->device));
  BivfWrite w(h);
  hipStream_t s = h->defctx->own;
  Scoped<float> d_rows;
  auto body = [&]() -> int {
    ZRET(d_rows.alloc((size_t)n * dim));
    ZCHK(hipMemcpyAsync(d_rows, rows, (size_t)n * dim * 4, hipMemcpyHostToDevice, s));
    return bivf_build_fp32_locked(w, d_rows, n, dim, metric, keys, nlist, kmeans_iters, seed, bin_threshold, s);
  };
  return w.done(body(), s);                // (synchronises before d_rows goes)
}

// rows: [count][dim] in list order, host or device (hipMemcpyDefault tells).  The new array takes the old one's place only once it
// is complete.
static int bivf_attach_rows(zvec_hip_bivf_t h, const float *rows, uint32_t dim, int metric, hipStream_t stream, bool own_stream) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZRET(bivf_fp32_pairs(h, dim, metric));
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::unique_lock<FairSharedMutex> wr(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (h->count && !rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = own_stream ? h->defctx->own : stream;
  Scoped<float> fresh;
  ZRET(fresh.alloc(std::max<size_t>((size_t)h->count * dim, 1)));
  if (h->count) ZCHK(hipMemcpyAsync(fresh, rows, (size_t)h->count * dim * 4, hipMemcpyDefault, s));
  ZCHK(hipStreamSynchronize(s));
  h->frows = std::move(fresh);             // (the old rows go with `fresh`)
  h->fdim = dim;
  h->fmetric = metric;
  return 0;
}

int zvec_hip_bivf_attach_rows(zvec_hip_bivf_t h, const float *rows, uint32_t dim, int metric) {
  return bivf_attach_rows(h, rows, dim, metric, nullptr, true);
}

int zvec_hip_bivf_attach_rows_dev(zvec_hip_bivf_t h, const float *d_rows, uint32_t dim, int metric, void *stream) {
  return bivf_attach_rows(h, d_rows, dim, metric, reinterpret_cast<hipStream_t>(stream), stream == nullptr);
}

int zvec_hip_bivf_get_rows(zvec_hip_bivf_t h, const uint64_t *list_positions, uint64_t n, float *out) {
  if (!h || (n && (!list_positions || !out))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (h->fdim == 0) return ZVEC_HIP_ERR_NO_READY;
  for (uint64_t i = 0; i < n; ++i)
    if (list_positions[i] >= h->count) return ZVEC_HIP_ERR_NO_EXIST;
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = h->defctx->own;
  Scoped<uint64_t> d_pos;
  Scoped<float> d_out;
  ZRET(d_pos.alloc(n));
  ZRET(d_out.alloc((size_t)n * h->fdim));
  ZCHK(hipMemcpyAsync(d_pos, list_positions, (size_t)n * 8, hipMemcpyHostToDevice, s));
  ZRET(launch_gather_f32_rows(h->frows, d_pos, n, h->fdim, d_out, s));
  ZCHK(hipMemcpyAsync(out, d_out, (size_t)n * h->fdim * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipStreamSynchronize(s));
  return 0;
}

int zvec_hip_bivf_rows_info(zvec_hip_bivf_t h, uint32_t *dim, int *metric, uint64_t *bytes) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  const bool on = h->loaded && h->fdim != 0;
  if (dim) *dim = on ? h->fdim : 0;
  if (metric) *metric = on ? h->fmetric : 0;
  if (bytes) *bytes = on ? (uint64_t)h->count * h->fdim * 4 : 0;
  return 0;
}

// what can be refused without the handle's state
static int bivf_search_fp32_args(zvec_hip_bivf_t h, const void *queries, uint32_t topk, uint32_t refine, uint32_t nprobe, const void *keys,
                                 const void *scores, const void *counts) {
  if (!h || !queries || !keys || !scores || !counts) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (topk == 0 || refine == 0 || nprobe == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return topk > BIVF_RERANK_MAX_KC ? ZVEC_HIP_ERR_UNSUPPORTED : 0;
}
// ... and with it (h->rw held)
static int bivf_search_fp32_state(const zvec_hip_bivf_s *h, uint32_t dim) {
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (h->fdim == 0) return ZVEC_HIP_ERR_NO_READY;
  if (dim != h->fdim) return ZVEC_HIP_ERR_MISMATCH;
  return dim > BIVF_RERANK_MAX_DIM ? ZVEC_HIP_ERR_UNSUPPORTED : 0;
}
static uint32_t bivf_rerank_kc(uint32_t topk, uint32_t refine) {
  return (uint32_t)std::min<uint64_t>((uint64_t)topk * refine, BIVF_RERANK_MAX_KC);
}

// both stages for fp32 DEVICE queries; the caller holds c->mu and h->rw (shared) and has validated everything
static int bivf_search_fp32_locked(zvec_hip_bivf_s *h, zvec_hip_ctx_s *c, const float *d_queries, uint32_t count, uint32_t dim, uint32_t topk,
                                   uint32_t refine, float threshold, float bin_threshold, uint32_t nprobe, uint32_t max_scan_count,
                                   const uint64_t *d_exclude, uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, hipStream_t s) {
  ZRET(c->benc.ensure((size_t)count * benc_words(dim) * 4));
  ZRET(launch_binary_encode(d_queries, count, dim, dim, bin_threshold, c->benc.as<uint32_t>(), s));
  const BivfRerank rr{d_queries, dim, topk, threshold};
  return bivf_search_dev_locked(h, c, c->benc.p, count, bivf_rerank_kc(topk, refine), FLT_MAX, nprobe, max_scan_count, d_exclude, d_out_keys,
                                d_out_scores, d_out_counts, s, &rr);
}

int zvec_hip_bivf_search_fp32_dev(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const float *d_queries, uint32_t count, uint32_t dim, uint32_t topk,
                                  uint32_t refine, float threshold, float bin_threshold, uint32_t nprobe, uint32_t max_scan_count,
                                  const uint64_t *d_exclude_bitset, uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts,
                                  void *stream) {
  ZRET(bivf_search_fp32_args(h, d_queries, topk, refine, nprobe, d_out_keys, d_out_scores, d_out_counts));
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  ZRET(bivf_search_fp32_state(h, dim));
  if (count == 0) return 0;
  ZCHK(hipSetDevice(h->device));
  return bivf_search_fp32_locked(h, c, d_queries, count, dim, topk, refine, threshold, bin_threshold, nprobe, max_scan_count, d_exclude_bitset,
                                 d_out_keys, d_out_scores, d_out_counts, pick_stream(c, stream));
}

// host_search_wrap_end for outputs of which only the first counts[q] entries of a row were written: nothing else of the caller's
// rows is touched
static int bivf_copy_out_counted(zvec_hip_ctx_s *ctx, uint32_t count, uint32_t topk, uint64_t *out_keys, float *out_scores, uint32_t *out_counts,
                                 hipStream_t stream) {
  const size_t kb = (size_t)count * topk * sizeof(uint64_t), sb = ((size_t)count * topk * sizeof(float) + 15) & ~(size_t)15,
               cb = (size_t)count * sizeof(uint32_t);
  const char *src = nullptr;
  std::vector<char> big;
  if (ctx->out_mapped) {
    ZRET(host_wait(ctx, stream));
    src = static_cast<const char *>(ctx->pin_out.p);
  } else {
    char *dst = nullptr;
    if (kb + sb + cb <= PIN_LIMIT && ctx->pin_out.ensure(kb + sb + cb) == 0) dst = static_cast<char *>(ctx->pin_out.p);
    else { big.resize(kb + sb + cb); dst = big.data(); }
    ZCHK(hipMemcpyAsync(dst, ctx->io_out.p, kb + sb + cb, hipMemcpyDeviceToHost, stream));
    ZRET(host_wait(ctx, stream));
    src = dst;
  }
  const uint64_t *keys = reinterpret_cast<const uint64_t *>(src);
  const float *scores = reinterpret_cast<const float *>(src + kb);
  const uint32_t *counts = reinterpret_cast<const uint32_t *>(src + kb + sb);
  for (uint32_t q = 0; q < count; ++q) {
    const uint32_t n = std::min(counts[q], topk);
    memcpy(out_keys + (size_t)q * topk, keys + (size_t)q * topk, (size_t)n * 8);
    memcpy(out_scores + (size_t)q * topk, scores + (size_t)q * topk, (size_t)n * 4);
    out_counts[q] = n;
  }
  return 0;
}

int zvec_hip_bivf_search_fp32(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const float *queries, uint32_t count, uint32_t dim, uint32_t topk,
                              uint32_t refine, float threshold, float bin_threshold, uint32_t nprobe, uint32_t max_scan_count,
                              const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores, uint32_t *out_counts) {
  ZRET(bivf_search_fp32_args(h, queries, topk, refine, nprobe, out_keys, out_scores, out_counts));
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);                // one critical section from the upload to the copy-out (zvec_hip_bivf_search)
  {
    std::shared_lock<FairSharedMutex> r(h->rw);
    ZRET(bivf_search_fp32_state(h, dim));
    if (count == 0) return 0;
    ZCHK(hipSetDevice(h->device));
    ZRET(host_search_wrap_begin(c, queries, (size_t)count * dim * 4, exclude_bitset, h->count, count, topk, c->cur));
    ZRET(bivf_search_fp32_locked(h, c, static_cast<const float *>(c->io_qp), count, dim, topk, refine, threshold, bin_threshold, nprobe,
                                 max_scan_count, exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr, c->io_keys.as<uint64_t>(),
                                 c->io_scores.as<float>(), c->io_counts.as<uint32_t>(), c->cur));
  }
  return bivf_copy_out_counted(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

int zvec_hip_bivf_last_candidates(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t kc, uint32_t *positions,
                                  float *hamming_scores, uint32_t *counts) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->bivf_owner != h || c->bivf_cand_count == 0 || count > c->bivf_cand_count || kc != c->bivf_cand_kc) return ZVEC_HIP_ERR_NO_READY;
  ZCHK(hipSetDevice(h->device));
  ZCHK(hipStreamSynchronize(c->cur));
  const BivfCand b = bivf_cand_arrays(c, c->bivf_cand_count, kc, c->bivf_cand_slice);
  if (positions) ZCHK(hipMemcpy(positions, b.pos, (size_t)count * kc * 4, hipMemcpyDeviceToHost));
  if (hamming_scores) ZCHK(hipMemcpy(hamming_scores, b.scores, (size_t)count * kc * 4, hipMemcpyDeviceToHost));
  if (counts) ZCHK(hipMemcpy(counts, b.counts, (size_t)count * 4, hipMemcpyDeviceToHost));
  return 0;
}
