// api_entry_int8_quant.inc.h — C ABI entry points: fp32 -> int8 on the device (Int8QuantizerReformer's two transforms), what feeds an
// int8 HNSW handle (zvec_hip_hnsw_create_typed with ZVEC_HIP_DT_INT8) with rows and queries (inside extern "C").  Device code:
// int8_encode_kernel, zvk_hnsw_i8.hip.h.  The shape of zvec_hip_binary_encode[_dev] beside it (api_entry_binary_quant.inc.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

namespace {

inline bool i8enc_args_ok(uint32_t dim, int mode, float scale) {
  if (dim == 0 || dim > BENC_MAX_DIM) return false;
  return mode == ZVEC_HIP_INT8_PER_ROW || (mode == ZVEC_HIP_INT8_SCALE_BIAS && scale > 0.f);      // (a nan scale fails the comparison)
}

// [count][dim] fp32 -> [count][dim] int8 and, per_row with d_factors, [count] factors; enqueued on `s` (arguments validated, count != 0)
int launch_int8_encode(const float *d_in, uint64_t count, uint32_t dim, int mode, float scale, float bias, int8_t *d_out, float *d_factors,
                       hipStream_t s) {
  const unsigned blocks = (unsigned)std::min<uint64_t>((count + 3) / 4, 1u << 16);      // (the waves stride over the rows)
  hipLaunchKernelGGL(int8_encode_kernel, dim3(blocks), dim3(256), 0, s, d_in, count, dim, mode == ZVEC_HIP_INT8_PER_ROW ? 1 : 0, scale, bias,
                     d_out, d_factors);
  ZCHK(hipGetLastError());
  return 0;
}

}  // namespace

int zvec_hip_int8_encode_dev(zvec_hip_ctx_t ctx, const float *d_in, uint64_t count, uint32_t dim, int mode, float scale, float bias,
                             int8_t *d_out, float *d_out_factors, void *stream) {
  if (!ctx || !i8enc_args_ok(dim, mode, scale)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!d_in || !d_out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ZCHK(hipSetDevice(ctx->device));
  return launch_int8_encode(d_in, count, dim, mode, scale, bias, d_out, d_out_factors, pick_stream(ctx, stream));
}

int zvec_hip_int8_encode(zvec_hip_ctx_t ctx, const float *in, uint64_t count, uint32_t dim, int mode, float scale, float bias, int8_t *out,
                         float *out_factors) {
  if (!ctx || !i8enc_args_ok(dim, mode, scale)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!in || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(ctx->mu);
  ZCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->cur;
  const bool fac = mode == ZVEC_HIP_INT8_PER_ROW && out_factors;
  const uint64_t rows_per = std::max<uint64_t>(1, BENC_SLICE_BYTES / ((uint64_t)dim * 4));
  DevBuf d_in, d_out, d_fac;
  for (uint64_t o = 0; o < count; o += rows_per) {
    const uint64_t m = std::min(rows_per, count - o);
    ZRET(d_in.ensure((size_t)m * dim * 4));
    ZRET(d_out.ensure((size_t)m * dim));
    if (fac) ZRET(d_fac.ensure((size_t)m * 4));
    ZCHK(hipMemcpyAsync(d_in.p, in + (size_t)o * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, s));
    ZRET(launch_int8_encode(d_in.as<float>(), m, dim, mode, scale, bias, d_out.as<int8_t>(), fac ? d_fac.as<float>() : nullptr, s));
    ZCHK(hipMemcpyAsync(out + (size_t)o * dim, d_out.p, (size_t)m * dim, hipMemcpyDeviceToHost, s));
    if (fac) ZCHK(hipMemcpyAsync(out_factors + o, d_fac.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    ZCHK(hipStreamSynchronize(s));
  }
  return 0;
}
