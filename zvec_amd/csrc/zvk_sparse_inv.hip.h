// zvk_sparse_inv.hip.h — sparse rows under InnerProductSparse through a term-major twin of the CSR rows (inverted lists): the tile pass.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// The row scan of zvk_sparse.hip.h visits every stored element for every query block, although a row contributes to an inner
// product only through indices the query has as well.  The twin (zvec_hip_sparse_set_inverted) holds the same elements by index:
//   terms[nterms]          the distinct stored indices, ascending (indices span 32 bits: a sorted table, no dense directory)
//   list_off[nterms + 1]   u64 posting offsets
//   ppos[elements]         u32 storage position of every posting, ascending inside a list
//   pval[elements]         its value in the handle's type (VT; halves stay halves and are widened where they are read)
//
// Tile pass.  ONE wave per work-group; a work item is (query, tile of SPARSE_INV_TILE consecutive positions) and owns one fp32
// accumulator per position of its tile in LDS, zeroed at the start.  The query's run is taken 64 terms at a time: lane = term
// looks its index up in terms[] (lower bound, at most ceil(log2(nterms + 1)) probes; an absent index leaves an empty range), then
// lower-bounds the tile's first and one-past-last position in its list, so that the range [s, e) of every term is known before
// anything is walked and is bounded by the list's own ends, never by the data.  Then the terms are walked ONE AFTER THE OTHER in
// run order (wave-uniform, the ranges broadcast): lane = posting, 256 postings in flight, acc[pos - tile0] = fmaf(value, q_value,
// acc[pos - tile0]).  Positions inside one list are distinct, so the lanes of one term never meet in an accumulator and a plain
// LDS read-modify-write is race-free; a fence between terms orders the next term's reads behind this term's writes.  No atomics
// anywhere: a row's sum is the fmaf chain over its shared indices in the query's run order (ascending for a valid run), the same
// bits on every call.  Afterwards the item writes sparse_score<false>(acc) = 0.f - acc into the dense [query][position] matrix
// that merge_kernel selects from, +inf for an excluded position and for the padding behind the last row.
//
// zvec_hip_sparse_search_dev cannot see its queries: an index that repeats is walked twice, one that descends is still found
// (each term is looked up on its own), nothing is read out of range, and every accumulator index is checked against the tile.
#pragma once
#include "zvk_sparse.hip.h"

namespace zvk {

constexpr uint32_t SPARSE_INV_TILE = 4096;     // positions per work item: 16 KiB of accumulators (DESIGN §3b "Inverted lists")

struct SparseInvArgs {
  const uint32_t *terms;      // [nterms]
  const uint64_t *list_off;   // [nterms + 1]
  const uint32_t *ppos;       // [elements]
  const void *pval;           // [elements] of the kernel's VT
  uint32_t nterms;
  const uint32_t *exclude;    // nullable bitset over positions, set = skip
  const uint32_t *q_off;      // [nq + 1] element offsets of the queries in q_idx / q_val
  const uint32_t *q_idx;
  const void *q_val;          // VT as well
  uint32_t q0;                // the query whose scores are row 0 of `out`
  uint32_t nq;                // queries of this launch: q0 .. q0 + nq
  uint64_t n;                 // rows
  uint32_t stride;            // floats per row of `out`: whole tiles, >= n
  float *out;                 // [nq][stride]
};

// first e in [lo, hi) with ppos[e] >= x, hi if there is none
__device__ __forceinline__ uint64_t sparse_inv_lower_bound(const uint32_t *ppos, uint64_t lo, uint64_t hi, uint32_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (ppos[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename VT, bool EXCL>
__global__ void __launch_bounds__(64) sparse_inv_kernel(const SparseInvArgs a) {
  extern __shared__ f32x4 zvk_smem4[];
  float *acc = reinterpret_cast<float *>(zvk_smem4);                  // [SPARSE_INV_TILE]
  const int lane = threadIdx.x;
  const VT *pval = static_cast<const VT *>(a.pval), *q_val = static_cast<const VT *>(a.q_val);
  // (the queries of one tile are neighbours in the grid: they walk the same stretch of the hot lists)
  const uint32_t tile = blockIdx.x / a.nq, qs = blockIdx.x - tile * a.nq, q = a.q0 + qs;
  const uint32_t tile0 = tile * SPARSE_INV_TILE;                      // (stride fits 32 bits, so does every tile's end)
  for (uint32_t i = (uint32_t)lane * 4; i < SPARSE_INV_TILE; i += 256) *reinterpret_cast<f32x4 *>(acc + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();

  const uint32_t qb = a.q_off[q], qlen = min(a.q_off[q + 1] - qb, SPARSE_MAX_COUNT);
  for (uint32_t b = 0; b < qlen; b += 64) {
    // lane = term: where its postings of this tile lie
    uint64_t s = 0, e = 0;
    float qv = 0.f;
    if (b + (uint32_t)lane < qlen) {
      const uint32_t t = a.q_idx[qb + b + lane];
      qv = (float)q_val[qb + b + lane];                               // (a half widens exactly)
      uint32_t lo = 0, hi = a.nterms;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.terms[mid] < t) lo = mid + 1;
        else hi = mid;
      }
      if (lo < a.nterms) {
        if (a.terms[lo] == t) {
          const uint64_t l1 = a.list_off[lo + 1];
          s = sparse_inv_lower_bound(a.ppos, a.list_off[lo], l1, tile0);
          e = sparse_inv_lower_bound(a.ppos, s, l1, tile0 + SPARSE_INV_TILE);
        }
      }
    }
    // the terms one after the other, lane = posting
    const uint32_t m = min(64u, qlen - b);
    for (uint32_t j = 0; j < m; ++j) {                                // (uniform)
      const uint64_t sj = bcast_u64(s, (int)j), ej = bcast_u64(e, (int)j);
      if (sj >= ej) continue;
      const float qj = bcast_f(qv, (int)j);
      for (uint64_t p = sj; p < ej; p += 256) {
        uint32_t r[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint64_t pe = p + (uint64_t)u * 64 + (uint32_t)lane;
          const bool in = pe < ej;
          r[u] = in ? a.ppos[pe] - tile0 : SPARSE_INV_TILE;
          v[u] = in ? (float)pval[pe] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (r[u] < SPARSE_INV_TILE) acc[r[u]] = __builtin_fmaf(v[u], qj, acc[r[u]]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // four positions per lane and store: they share one word of the bitset
  float *out = a.out + (size_t)qs * a.stride + tile0;
  for (uint32_t i = (uint32_t)lane * 4; i < SPARSE_INV_TILE; i += 256) {
    const f32x4 sum = *reinterpret_cast<const f32x4 *>(acc + i);
    const uint64_t pos = (uint64_t)tile0 + i;
    uint32_t ex = 0;
    if (EXCL) {
      if (pos < a.n) ex = a.exclude[pos >> 5] >> (pos & 31);
    }
    f32x4 sc;
#pragma unroll
    for (int u = 0; u < 4; ++u) sc[u] = (pos + u < a.n && ((ex >> u) & 1u) == 0) ? sparse_score<false>(sum[u], 0.f, 0u, 0u, 0.f) : __builtin_inff();
    *reinterpret_cast<f32x4 *>(out + i) = sc;
  }
}

}  // namespace zvk
