// api_entry_binary_quant.inc.h — C ABI entry points: fp32 -> sign bits on the device (BinaryConverter / BinaryReformer), and the
// flat Hamming index fed with fp32 rows and fp32 queries (inside extern "C")
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

namespace {

constexpr uint32_t BENC_MAX_DIM = 1u << 20;            // the cap of a binary handle's bit width (zvec_hip_flat_create)
constexpr uint64_t BENC_SLICE_BYTES = 64ull << 20;     // fp32 bytes staged per slice of a host-pointer call; words kept per slice of an append

inline uint32_t benc_words(uint32_t dim) { return (dim + 31) / 32; }

inline bool benc_args_ok(uint32_t dim, uint32_t encode_dims) {
  return dim != 0 && dim <= BENC_MAX_DIM && encode_dims != 0 && encode_dims <= dim;
}

// [count][dim] fp32 -> [count][ceil(dim / 32)] words, enqueued on `s` (arguments validated, count != 0)
int launch_binary_encode(const float *d_in, uint64_t count, uint32_t dim, uint32_t encode_dims, float threshold, uint32_t *d_out, hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<uint64_t>((count + 3) / 4, 1u << 16);      // (the waves stride over the rows)
  hipLaunchKernelGGL(binary_encode_kernel, dim3(blocks), dim3(256), 0, s, d_in, count, dim, encode_dims, threshold, d_out);
  ZCHK(hipGetLastError());
  return 0;
}

// the converter only ever emits DT_BINARY32 rows of 32 * ceil(dim / 32) bits (binary_converter.cc:93-102)
inline bool benc_handle_pairs(const zvec_hip_flat_s *h, uint32_t dim) {
  return h->dtype == ZVEC_HIP_DT_BINARY32 && h->st.dim_in == benc_words(dim) * 32u;
}

// `m` fp32 device rows -> sign bits -> the store, through h->enc in slices; the caller is inside a FlatWrite on `s` and has
// reserved the store for the rows
int flat_append_encoded(zvec_hip_flat_s *h, const float *d_rows, uint64_t m, uint32_t dim, uint32_t encode_dims, float threshold,
                        const uint64_t *d_keys, hipStream_t s) {
  const uint32_t words = benc_words(dim);
  const uint64_t rows_per = std::max<uint64_t>(1, BENC_SLICE_BYTES / ((uint64_t)words * 4));
  ZRET(h->enc.ensure((size_t)std::min(rows_per, m) * words * 4));       // (growing frees the old block, which waits for the device)
  for (uint64_t o = 0; o < m; o += rows_per) {
    const uint64_t c = std::min(rows_per, m - o);
    ZRET(launch_binary_encode(d_rows + (size_t)o * dim, c, dim, encode_dims, threshold, h->enc.as<uint32_t>(), s));
    ZRET(store_append_dev(h->st, h->enc.p, c, d_keys ? d_keys + o : nullptr, s));
  }
  return 0;
}

}  // namespace

int zvec_hip_binary_encode_dev(zvec_hip_ctx_t ctx, const float *d_in, uint64_t count, uint32_t dim, uint32_t encode_dims, float threshold,
                               uint32_t *d_out, void *stream) {
  if (!ctx || !benc_args_ok(dim, encode_dims)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!d_in || !d_out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ZCHK(hipSetDevice(ctx->device));
  return launch_binary_encode(d_in, count, dim, encode_dims, threshold, d_out, pick_stream(ctx, stream));
}

int zvec_hip_binary_encode(zvec_hip_ctx_t ctx, const float *in, uint64_t count, uint32_t dim, uint32_t encode_dims, float threshold,
                           uint32_t *out) {
  if (!ctx || !benc_args_ok(dim, encode_dims)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!in || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ZCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->cur;
  const uint32_t words = benc_words(dim);
  const uint64_t rows_per = std::max<uint64_t>(1, BENC_SLICE_BYTES / ((uint64_t)dim * 4));
  DevBuf d_in, d_out;
  for (uint64_t o = 0; o < count; o += rows_per) {
    const uint64_t m = std::min(rows_per, count - o);
    ZRET(d_in.ensure((size_t)m * dim * 4));
    ZRET(d_out.ensure((size_t)m * words * 4));
    ZCHK(hipMemcpyAsync(d_in.p, in + (size_t)o * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, s));
    ZRET(launch_binary_encode(d_in.as<float>(), m, dim, encode_dims, threshold, d_out.as<uint32_t>(), s));
    ZCHK(hipMemcpyAsync(out + (size_t)o * words, d_out.p, (size_t)m * words * 4, hipMemcpyDeviceToHost, s));
    ZCHK(hipStreamSynchronize(s));
  }
  return 0;
}

int zvec_hip_flat_append_fp32_dev(zvec_hip_flat_t h, const float *d_vecs, uint64_t n, uint32_t dim, uint32_t encode_dims, float threshold,
                                  const uint64_t *d_keys, void *stream) {
  if (!h || !benc_args_ok(dim, encode_dims)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (!benc_handle_pairs(h, dim)) return ZVEC_HIP_ERR_MISMATCH;
  if (n == 0) return 0;
  if (!d_vecs) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  FlatWrite w(h);
  ZRET(w.open(stream));
  // everything that can refuse comes before the first row is stored: all of the rows or none
  ZRET(w.cover(h->st.n + n));
  ZRET(h->st.reserve(h->st.n + n, w.s));
  return w.finish_enqueued(flat_append_encoded(h, d_vecs, n, dim, encode_dims, threshold, d_keys, w.s));
}

int zvec_hip_flat_append_fp32(zvec_hip_flat_t h, const float *vecs, uint64_t n, uint32_t dim, uint32_t encode_dims, float threshold,
                              const uint64_t *keys) {
  if (!h || !benc_args_ok(dim, encode_dims)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (!benc_handle_pairs(h, dim)) return ZVEC_HIP_ERR_MISMATCH;
  if (n == 0) return 0;
  if (!vecs) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  FlatWrite w(h);
  ZRET(w.open());
  hipStream_t s = w.s;
  ZRET(w.cover(h->st.n + n));
  ZRET(h->st.reserve(h->st.n + n, s));
  const uint64_t rows_per = std::max<uint64_t>(1, BENC_SLICE_BYTES / ((uint64_t)dim * 4));
  DevBuf tmp, tk;
  ZRET(tmp.ensure((size_t)std::min(rows_per, n) * dim * 4));
  if (keys) ZRET(tk.ensure((size_t)std::min(rows_per, n) * 8));
  auto slices = [&]() -> int {
    for (uint64_t o = 0; o < n; o += rows_per) {
      const uint64_t m = std::min(rows_per, n - o);
      ZCHK(hipMemcpyAsync(tmp.p, vecs + (size_t)o * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, s));
      if (keys) ZCHK(hipMemcpyAsync(tk.p, keys + o, (size_t)m * 8, hipMemcpyHostToDevice, s));
      ZRET(flat_append_encoded(h, tmp.as<float>(), m, dim, encode_dims, threshold, keys ? tk.as<uint64_t>() : nullptr, s));
      ZCHK(hipStreamSynchronize(s));
    }
    return 0;
  };
  return w.finish_synced(slices());
}

int zvec_hip_flat_search_fp32_dev(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const float *d_queries, uint32_t dim, float bin_threshold,
                                  uint32_t count, uint32_t topk, float threshold, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                                  float *d_out_scores, uint32_t *d_out_counts, void *stream) {
  if (!h || !d_queries || !d_out_keys || !d_out_scores || !d_out_counts || !benc_args_ok(dim, dim)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (!benc_handle_pairs(h, dim)) return ZVEC_HIP_ERR_MISMATCH;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = pick_stream(c, stream);
  ZRET(c->benc.ensure((size_t)count * benc_words(dim) * 4));
  ZRET(launch_binary_encode(d_queries, count, dim, dim, bin_threshold, c->benc.as<uint32_t>(), s));
  return flat_search_dev_locked(h, c, c->benc.p, count, topk, threshold, d_exclude_bitset, d_out_keys, d_out_scores, d_out_counts, s);
}

int zvec_hip_flat_search_fp32(zvec_hip_flat_t h, zvec_hip_ctx_t ctx, const float *queries, uint32_t dim, float bin_threshold, uint32_t count,
                              uint32_t topk, float threshold, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                              uint32_t *out_counts) {
  if (!h || !queries || !out_keys || !out_scores || !out_counts || !benc_args_ok(dim, dim)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (!benc_handle_pairs(h, dim)) return ZVEC_HIP_ERR_MISMATCH;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);              // one critical section from the upload to the copy-out (zvec_hip_flat_search)
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw);
    ZRET(host_search_wrap_begin(c, queries, (size_t)count * dim * 4, exclude_bitset, h->st.n, count, topk, c->cur));
    ZRET(c->benc.ensure((size_t)count * benc_words(dim) * 4));
    ZRET(launch_binary_encode(static_cast<const float *>(c->io_qp), count, dim, dim, bin_threshold, c->benc.as<uint32_t>(), c->cur));
    ZRET(flat_search_dev_locked(h, c, c->benc.p, count, topk, threshold, exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr,
                                c->io_keys.as<uint64_t>(), c->io_scores.as<float>(), c->io_counts.as<uint32_t>(), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}
