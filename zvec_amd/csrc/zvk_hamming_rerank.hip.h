// zvk_hamming_rerank.hip.h — the fp32 side of a Hamming IVF index: the gather of the fp32 rows into list order, and the re-rank of
// a query's Hamming candidates on those rows.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Reference: the pipeline BinaryConverter (src/core/quantizer/binary_converter.cc:25-128) -> IVFBuilder (ivf_builder.cc:212-403) ->
// BinaryReformer (binary_reformer.cc:46-68) -> IVFStreamer::search_impl (ivf_streamer.cc:183-250) ends with Hamming scores; a
// deployment re-scores the survivors on the values the bits were made from.  That step lives here, on the device.
//
// Layout.  The fp32 rows are one plain row-major array [count][dim] beside the binary Store of zvk_hamming_ivf.hip.h: row p is the
// document at list-order position p, so a candidate's position addresses both.
#pragma once
#include "zvk_common.hip.h"

namespace zvk {

constexpr uint32_t BIVF_RERANK_MAX_KC = 128;          // candidates per query: all of their scores are ranked in LDS at once
// The query is staged once in the dynamic LDS of its work-group, followed by the 128 scores and the counter (528 bytes).  A launch
// may take 64 KiB of dynamic LDS without a raised limit: 63 KiB of query, dim <= 16128.
constexpr uint32_t BIVF_RERANK_MAX_DIM = 63 * 1024 / 4;
__host__ __device__ inline uint32_t bivf_rerank_qfloats(uint32_t dim) { return (dim + 3) & ~3u; }      // (keeps what follows 16-byte aligned)
__host__ __device__ inline size_t bivf_rerank_lds_bytes(uint32_t dim) {
  return (size_t)bivf_rerank_qfloats(dim) * 4 + BIVF_RERANK_MAX_KC * 4 + 16;
}

// ---- gather into list order -----------------------------------------------------------------------------------------------------
// dst[p] = src[perm[p]] for rows of `dim` floats: one wave per destination row, the lanes striding along it, so every load and store
// instruction of a wave covers 64 x 16 B (both arrays 16-byte aligned and dim % 4 == 0) or 64 x 4 B contiguous bytes.
__global__ void __launch_bounds__(256) bivf_gather_f32_rows_kernel(const float *src, const uint64_t *perm, uint64_t n, uint32_t dim, float *dst) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t p = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const float *s = src + (size_t)perm[p] * dim;
  float *d = dst + (size_t)p * dim;
  const bool vec = (dim & 3u) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  if (vec) {
    const f32x4 *s4 = reinterpret_cast<const f32x4 *>(s);
    f32x4 *d4 = reinterpret_cast<f32x4 *>(d);
    for (uint32_t i = lane; i < dim / 4; i += 64) d4[i] = s4[i];
  } else {
    for (uint32_t i = lane; i < dim; i += 64) d[i] = s[i];
  }
}

// ---- re-rank --------------------------------------------------------------------------------------------------------------------
struct BivfRerankArgs {
  const float *rows;              // [count][dim] fp32 rows in list order
  const float *queries;           // [nq][dim]
  const uint32_t *cand;           // [nq][kc] list-order positions, ascending by Hamming score (IDX_NONE: no candidate)
  const uint32_t *cand_cnt;       // [nq] candidates of each query
  const uint64_t *keymap;         // position -> key
  uint32_t dim, kc, topk;         // kc <= BIVF_RERANK_MAX_KC, topk <= kc
  uint32_t ip;                    // 0: squared L2, 1: minus the inner product
  float threshold;                // <= FLT_MAX
  uint64_t *out_keys;             // [nq][topk]
  float *out_scores;              // [nq][topk]
  uint32_t *out_counts;           // [nq]
};

// one term of a lane's sum: L2 rounds the difference once, then one fma; IP is one fma
template <bool IP>
__device__ __forceinline__ float rerank_term(float q, float b, float acc) {
  if constexpr (IP) return __builtin_fmaf(q, b, acc);
  const float d = q - b;
  return __builtin_fmaf(d, d, acc);
}

// the score of one row against the staged query, the same in every lane.  VEC: 16-byte loads (dim % 4 == 0, aligned rows).  Four
// loads of a lane are issued before the first fma; a lane keeps one sum per load slot and adds the four at the end.
template <bool IP, bool VEC>
__device__ __forceinline__ float rerank_row(const float *row, const float *Q, uint32_t dim, uint32_t lane) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    const f32x4 *r4 = reinterpret_cast<const f32x4 *>(row);
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(Q);
    const uint32_t nv = dim / 4;
    for (uint32_t i0 = lane; i0 < nv; i0 += 256) {
      f32x4 v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + u * 64;
        v[u] = i < nv ? r4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + u * 64;
        if (i < nv) {
          const f32x4 qv = q4[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[u] = rerank_term<IP>(qv[e], v[u][e], acc[u]);
        }
      }
    }
  } else {
    for (uint32_t i0 = lane; i0 < dim; i0 += 256) {
      float v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + u * 64;
        v[u] = i < dim ? row[i] : 0.f;
      }
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t i = i0 + u * 64;
        if (i < dim) acc[u] = rerank_term<IP>(Q[i], v[u], acc[u]);
      }
    }
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
  return IP ? -s : s;
}

// One work-group of four waves per query.  The query's floats are staged once in LDS; wave w scores candidates w, w + 4, ...; a
// candidate beyond the query's count, or an IDX_NONE slot, scores +inf.  With every score in LDS, thread t takes candidate t: its place
// is the number of candidates with a smaller (score, rank in the candidate list) pair — unique, so the result is one well-defined
// sequence with no float atomics and no dependence on wave timing.  Candidates placed below topk and within the radius write their
// key and score at their place (the kept ones form a prefix: scores ascend with the place); nothing else of the output rows is
// written.  The count is summed with integer atomics in LDS.
template <bool IP>
__device__ __forceinline__ void bivf_rerank_body(const BivfRerankArgs &a) {
  extern __shared__ f32x4 zvk_smem4[];
  float *Q = reinterpret_cast<float *>(zvk_smem4);
  float *sc = Q + bivf_rerank_qfloats(a.dim);                   // [BIVF_RERANK_MAX_KC]
  uint32_t *kept = reinterpret_cast<uint32_t *>(sc + BIVF_RERANK_MAX_KC);
  const uint32_t q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t dim = a.dim, kc = min(a.kc, BIVF_RERANK_MAX_KC);
  const float *qsrc = a.queries + (size_t)q * dim;
  for (uint32_t i = threadIdx.x; i < dim; i += 256) Q[i] = qsrc[i];
  if (threadIdx.x == 0) *kept = 0;
  const uint32_t cnt = min(a.cand_cnt[q], kc);
  const uint32_t *cand = a.cand + (size_t)q * a.kc;
  __syncthreads();
  const bool vec = (dim & 3u) == 0 && (reinterpret_cast<uintptr_t>(a.rows) & 15u) == 0;
  for (uint32_t c = wave; c < kc; c += 4) {
    const uint32_t pos = c < cnt ? cand[c] : IDX_NONE;          // uniform in the wave
    float s = __builtin_inff();
    if (pos != IDX_NONE) {
      const float *row = a.rows + (size_t)pos * dim;
      s = vec ? rerank_row<IP, true>(row, Q, dim, lane) : rerank_row<IP, false>(row, Q, dim, lane);
    }
    if (lane == 0) sc[c] = s;
  }
  __syncthreads();
  const uint32_t t = threadIdx.x;
  bool keep = false;
  uint32_t place = 0;
  float s = __builtin_inff();
  if (t < kc) {
    s = sc[t];
    for (uint32_t j = 0; j < kc; ++j) {
      const float o = sc[j];
      place += (o < s || (o == s && j < t)) ? 1u : 0u;
    }
    keep = s < __builtin_inff() && place < a.topk && s <= a.threshold;
  }
  if (keep) {
    const size_t o = (size_t)q * a.topk + place;
    a.out_keys[o] = a.keymap[cand[t]];
    a.out_scores[o] = s;
  }
  const uint64_t m = __ballot(keep);
  if (lane == 0 && m) atomicAdd(kept, (uint32_t)__popcll(m));
  __syncthreads();
  if (t == 0) a.out_counts[q] = *kept;
}

__global__ void __launch_bounds__(256) bivf_rerank_kernel(const BivfRerankArgs a) {
  if (a.ip) bivf_rerank_body<true>(a);
  else bivf_rerank_body<false>(a);
}

}  // namespace zvk
