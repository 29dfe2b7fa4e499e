// zvk_hnsw_i8.hip.h — the distance step of the HNSW walk over int8 rows (zvec_hip_hnsw_create_typed with ZVEC_HIP_DT_INT8,
// api_entry_hnsw.inc.h), and the fp32 -> int8 quantiser that feeds such a handle (zvec_hip_int8_encode, api_entry_int8_quant.inc.h).
// The walk, the build and the group-by stages are those of zvk_hnsw.hip.h, zvk_hnsw_build.hip.h and zvk_hnsw_group.hip.h,
// instantiated for HnswRows<HNSW_I8>; this file is the scorer they take and HnswDenseKind<HNSW_I8>.  DESIGN §3c "int8 rows".
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Scores: L2 = (float)(int32) sum (row[i] - q[i])^2, IP = (float)(int32)(-sum row[i] * q[i]).  The sum is an exact 32-bit integer:
// values are the full -128 .. 127, a difference is at most 255 in magnitude, and with dim <= HNSW_MAX_DIM = 4096
// |sum| <= 4096 * 255^2 = 266 342 400 < 2^31.  The only rounding is the conversion of that integer to fp32, to nearest even.
//
// Stored rows are [n][wpad] uint32_t words of four int8 values each (little-endian: value i is byte i of the row), words = dim / 4
// rounded up to 4 and zero padded, so every row is 16-byte aligned and a lane loads one 16-byte chunk per step: the layout of the
// bit rows (zvk_hnsw_hamming.hip.h), whose loop and lane split (G lanes a row, G the smallest power of two >= chunks, at most 16,
// 64 / G rows in flight) this kind shares.  A 128-d row is 8 chunks and a 768-d row 48: the sixteen-lane fp32 split would idle half
// the lanes on the first.  The query, or the build's base or candidate row, is wpad words in LDS.  A zero is neutral under both
// metrics, so the padding of the row and of the staged query adds nothing.
//
// The arithmetic is the packed signed 8-bit dot product (v_dot4_i32_i8 / v_dot4c_i32_i8: four products and the accumulator summed
// in 32 bits, nothing saturated).  IP is one dot per word.  L2 is a.a - 2 a.q + q.q, three dots per word and nothing kept outside
// the loop; no byte is widened to fp32 and none is subtracted on its own.
#pragma once
#include "zvk_hnsw_hamming.hip.h"

namespace zvk {

__device__ __forceinline__ int hnsw_dot4(uint32_t a, uint32_t b, int acc) { return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false); }

// The per-chunk step of hnsw_chunk_distances for int8 values, sixteen of them a chunk.  The accumulator is the sum modulo 2^32,
// which is the sum (the bound above); L2 takes the cross term of a chunk on its own and subtracts it twice.
template <bool IP>
struct HnswI8Acc {
  __device__ __forceinline__ uint32_t add(u32x4 b, u32x4 x, uint32_t acc) const {
    const int cross = hnsw_dot4(b.w, x.w, hnsw_dot4(b.z, x.z, hnsw_dot4(b.y, x.y, hnsw_dot4(b.x, x.x, 0))));
    if constexpr (IP) return acc + (uint32_t)cross;
    int sq = (int)acc;
    sq = hnsw_dot4(b.x, b.x, sq); sq = hnsw_dot4(b.y, b.y, sq); sq = hnsw_dot4(b.z, b.z, sq); sq = hnsw_dot4(b.w, b.w, sq);
    sq = hnsw_dot4(x.x, x.x, sq); sq = hnsw_dot4(x.y, x.y, sq); sq = hnsw_dot4(x.z, x.z, sq); sq = hnsw_dot4(x.w, x.w, sq);
    return (uint32_t)sq - 2u * (uint32_t)cross;
  }
  __device__ __forceinline__ float score(uint32_t acc) const { return (float)(IP ? -(int)acc : (int)acc); }
};

// The scorer of the walk over int8 rows (the contract of HnswDenseScorer, zvk_hnsw.hip.h) against the words at qw in LDS.  The
// metric is the handle's: uniform over the launch.
struct HnswI8Scorer {
  const uint32_t *qw;
  __device__ __forceinline__ void operator()(const HnswArgs &a, const uint32_t *coll, float *cdist, uint32_t nc, int lane) const {
    if (a.ip) hnsw_chunk_distances_any(a, qw, coll, cdist, nc, lane, HnswI8Acc<true>());
    else hnsw_chunk_distances_any(a, qw, coll, cdist, nc, lane, HnswI8Acc<false>());
  }
};

template <>
struct HnswDenseKind<HNSW_I8> {
  typedef uint32_t lds;
  typedef HnswI8Scorer Scorer;
  static __device__ __forceinline__ uint32_t word(const void *p, size_t i) { return static_cast<const uint32_t *>(p)[i]; }
};

// ---- fp32 -> int8: what feeds an int8 handle --------------------------------------------------------------------------------------
// std::round(v), halves away from zero, for |v| <= 127, without adding 0.5 (which can round up a value just below a half):
// t = trunc(|v|) and |v| - t, the fraction, are both exact, and the result is t + 1 when the fraction is at least 0.5.
__device__ __forceinline__ int i8q_round_away(float v) {
  const float m = __builtin_fabsf(v), t = __builtin_truncf(m);
  const int k = (int)t + ((m - t) >= 0.5f ? 1 : 0);
  return v < 0.f ? -k : k;
}

// clamp to the reference's [MIN_VALUE, MAX_VALUE] = [-127, 127] of EntropyInt8Quantizer (ailego/algorithm/integer_quantizer.h:171),
// then round; nan, which the reference leaves undefined, gives 0
__device__ __forceinline__ int i8q_value(float x) {
  if (!(x == x)) return 0;
  x = x > 127.f ? 127.f : x < -127.f ? -127.f : x;
  return i8q_round_away(x);
}

__device__ __forceinline__ float i8q_scaled(float v, float bias, float scale, bool per_row) {
  // one add and one multiply, each rounded to fp32 on its own: never contracted into an fma
  if (per_row) return __fmul_rn(v, scale);
  return __fmul_rn(__fadd_rn(v, bias), scale);
}

// [count][dim] fp32 -> [count][dim] int8, one wave per row at a time, four rows a work-group.
//   per_row == 0: EntropyInt8Quantizer::encode (integer_quantizer.cc:348-354): out = round(clamp((v + bias) * scale, -127, 127)).
//   per_row != 0: Int8QuantizerReformer's inner-product query transform (integer_quantizer_reformer.cc:236-246): s = 127 / max|v|
//   of the row (an abs-max reduction over the wave; max is exact, so its order is free), out = round(v * s); factors[row], when
//   given, is max|v| / 127.  A row of zeros, where the reference divides by zero, gives zeros and the factor 0.
// A lane takes four consecutive values per step and writes them as one word where the bytes allow it (`out` 4-byte aligned and
// dim % 4 == 0: every row of an int8 handle); otherwise the bytes go one by one.  The input needs its natural 4-byte alignment only.
__global__ void __launch_bounds__(256) int8_encode_kernel(const float *in, uint64_t count, uint32_t dim, int per_row, float scale, float bias,
                                                          int8_t *out, float *factors) {
  const uint32_t lane = threadIdx.x & 63;
  const bool words = (dim & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < count; row += (uint64_t)gridDim.x * 4) {
    const float *src = in + (size_t)row * dim;
    int8_t *dst = out + (size_t)row * dim;
    float s = scale;
    if (per_row) {
      float mx = 0.f;
      for (uint32_t i = lane; i < dim; i += 64) mx = fmaxf(mx, __builtin_fabsf(src[i]));
      for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      s = mx > 0.f ? __fdiv_rn(127.f, mx) : 0.f;
      if (factors && lane == 0) factors[row] = mx > 0.f ? __fdiv_rn(mx, 127.f) : 0.f;
    }
    for (uint32_t i0 = lane * 4; i0 < dim; i0 += 256) {
      int q[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e)
        if (i0 + e < dim) q[e] = i8q_value(i8q_scaled(src[i0 + e], bias, s, per_row != 0));
      if (words) {
        *reinterpret_cast<uint32_t *>(dst + i0) = ((uint32_t)q[0] & 0xffu) | (((uint32_t)q[1] & 0xffu) << 8) |
                                                  (((uint32_t)q[2] & 0xffu) << 16) | ((uint32_t)q[3] << 24);
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
          if (i0 + e < dim) dst[i0 + e] = (int8_t)q[e];
      }
    }
  }
}

}  // namespace zvk
