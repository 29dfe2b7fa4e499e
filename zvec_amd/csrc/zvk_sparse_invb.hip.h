// zvk_sparse_invb.hip.h — the device build of the term-major twin of a sparse index (zvk_sparse_inv.hip.h searches it).
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// The twin is the stored elements in a STABLE order by index.  The elements stand in position order in the CSR arrays, so
// stability alone makes every posting list ascend by position: the sort carries (index, element ordinal) and no second key.
//
//   invb_or_kernel        OR of every stored index -> the number of 8-bit digit passes, ceil(bits(OR) / 8); a digit that is zero in
//                         every index above it is never sorted by
//   per pass (least significant digit first; pass 0 reads idx[] and takes the ordinal from the element's place):
//     invb_hist_kernel    digit counts of each work-group's INVB_BLOCK consecutive elements -> table[digit][work-group]
//     invb_scan_*         exclusive scan over the whole table (digit-major: all of digit 0's work-groups, then digit 1's, ...)
//     invb_scatter_kernel element -> table[digit][work-group] + its rank among the work-group's elements of the same digit
//   invb_expand_kernel    row_off -> the position of every element (a wave per row)
//   invb_scan_* <Heads>   heads sorted[i] != sorted[i - 1]: their count is nterms; terms[] and list_off[] are scattered by the scan
//   invb_gather_kernel    ppos[i] = position[ordinal[i]], pval[i] = the bits of val[ordinal[i]] (32- or 16-bit words, never converted)
//
// Rank inside a work-group (4 waves; wave w owns elements [w * 512, w * 512 + 512) of the block and takes them in 8 rounds of 64
// consecutive ones, lane = element).  Inside a round the lanes of equal digit are found by a match over the digit's 8 bits (eight
// ballots); a lane's rank is the popcount of its peers below it.  Across rounds a wave keeps its own running count per digit in LDS
// (read by every peer, advanced by the lowest one).  Across waves the counts are prefixed in wave order.  So the rank is the number
// of elements of the same digit in front of the element, in element order, and no atomic decides where anything lands: the same
// store gives the same bytes every time.  (The histogram counts with LDS atomics: a count does not depend on the order of arrival.)
#pragma once
#include "zvk_common.hip.h"

namespace zvk {

constexpr uint32_t INVB_THREADS = 256;                                   // 4 waves
constexpr uint32_t INVB_ROUNDS = 8;                                      // elements per lane
constexpr uint32_t INVB_WAVE_ELEMS = 64 * INVB_ROUNDS;                   // 512 consecutive elements per wave
constexpr uint32_t INVB_BLOCK = INVB_THREADS * INVB_ROUNDS;              // 2048 elements per work-group (block_elems)
constexpr uint32_t INVB_SCAN_ROUNDS = 4;
constexpr uint32_t INVB_SCAN_CHUNK = INVB_THREADS * 4 * INVB_SCAN_ROUNDS;   // 4096 words per work-group of the scan

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void invb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ---- OR of the indices ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(INVB_THREADS) invb_or_kernel(const uint32_t *idx, uint64_t elems, uint32_t *out) {
  uint32_t v = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * INVB_THREADS + threadIdx.x; i < elems; i += (uint64_t)gridDim.x * INVB_THREADS) v |= idx[i];
  for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicOr(out, v);                    // (an OR: the same word in any order)
}

// ---- digit counts ---------------------------------------------------------------------------------------------------------------
// table[digit * nblocks + block]
__global__ void __launch_bounds__(INVB_THREADS) invb_hist_kernel(const uint32_t *keys, uint64_t elems, uint32_t shift, uint32_t *table,
                                                                 uint32_t nblocks) {
  __shared__ uint32_t cnt[4][256];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int j = 0; j < 4; ++j) cnt[j][t] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)blockIdx.x * INVB_BLOCK + w * INVB_WAVE_ELEMS + lane;
#pragma unroll
  for (uint32_t r = 0; r < INVB_ROUNDS; ++r) {
    const uint64_t i = e0 + r * 64;
    if (i < elems) atomicAdd(&cnt[w][(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[(size_t)t * nblocks + blockIdx.x] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}

// ---- stable scatter by one digit ------------------------------------------------------------------------------------------------
// FIRST: the pairs are (idx[i], i) and `oin` is not read.  table: the scanned counts.
template <bool FIRST>
__global__ void __launch_bounds__(INVB_THREADS) invb_scatter_kernel(const uint32_t *kin, const uint32_t *oin, uint32_t *kout, uint32_t *oout,
                                                                    uint64_t elems, uint32_t shift, const uint32_t *table,
                                                                    uint32_t nblocks) {
  __shared__ uint32_t cnt[4][256];       // per wave and digit: the running count, afterwards the wave's first destination
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int j = 0; j < 4; ++j) cnt[j][t] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)blockIdx.x * INVB_BLOCK + w * INVB_WAVE_ELEMS + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t key[INVB_ROUNDS], ord[INVB_ROUNDS], off[INVB_ROUNDS];
#pragma unroll
  for (uint32_t r = 0; r < INVB_ROUNDS; ++r) {
    const uint64_t i = e0 + r * 64;
    const bool in = i < elems;
    key[r] = in ? kin[i] : 0u;
    ord[r] = FIRST ? (uint32_t)i : (in ? oin[i] : 0u);
  }
#pragma unroll
  for (uint32_t r = 0; r < INVB_ROUNDS; ++r) {
    const bool in = e0 + r * 64 < elems;
    const uint32_t d = (key[r] >> shift) & 255u;
    uint64_t peers = __ballot(in);                                       // (the lanes behind the last element match nobody)
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    const uint32_t prev = in ? cnt[w][d] : 0u;
    invb_wave_sync();
    if (in && rank == 0) cnt[w][d] = prev + (uint32_t)__popcll(peers);
    invb_wave_sync();
    off[r] = prev + rank;
  }
  __syncthreads();
  {                                                                      // thread = digit: the waves' counts -> their first destinations
    uint32_t g = table[(size_t)t * nblocks + blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t c = cnt[j][t];
      cnt[j][t] = g;
      g += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < INVB_ROUNDS; ++r) {
    if (e0 + r * 64 < elems) {
      const uint64_t dst = (uint64_t)cnt[w][(key[r] >> shift) & 255u] + off[r];
      if (dst < elems) {                                                 // (always, with a table scanned from this pass's counts)
        kout[dst] = key[r];
        oout[dst] = ord[r];
      }
    }
  }
}

// ---- exclusive scan of one 32-bit word per item (the totals fit: they count elements) ----------------------------------------
// An item is a word of an array (the count table, scanned in place) or a head flag of the sorted indices (the scan then writes
// terms[] and list_off[] instead of the prefix).  Three launches: the sum of every chunk, one work-group over the sums, the chunks.

// exclusive prefix of v over the work-group's threads; `total` is the sum, in every thread
__device__ __forceinline__ uint32_t invb_block_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
    if ((int)lane >= d) inc += o;
  }
  __syncthreads();                                                       // (the previous call's sums have been read)
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (uint32_t j = 0; j < INVB_THREADS / 64; ++j) {
    const uint32_t s = wsum[j];
    before += j < w ? s : 0u;
    tot += s;
  }
  total = tot;
  return before + inc - v;
}

struct InvbWords {
  uint32_t *p;                           // [n], 16-byte aligned
  __device__ __forceinline__ void load4(uint64_t i, uint64_t n, uint32_t v[4]) const {
    if (i + 4 <= n) {
      const u32x4 x = *reinterpret_cast<const u32x4 *>(p + i);
      v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = i + e < n ? p[i + e] : 0u;
    }
  }
  __device__ __forceinline__ void emit(uint64_t i, uint32_t, uint32_t prefix) const { p[i] = prefix; }
};

struct InvbHeads {
  const uint32_t *key;                   // [n] sorted indices
  uint32_t *terms;                       // [heads]
  uint64_t *list_off;                    // [heads + 1]; the caller writes the last one
  __device__ __forceinline__ void load4(uint64_t i, uint64_t n, uint32_t v[4]) const {
    uint32_t prev = (i > 0 && i < n) ? key[i - 1] : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = i + e < n;
      const uint32_t k = in ? key[i + e] : 0u;
      v[e] = (in && (i + e == 0 || k != prev)) ? 1u : 0u;
      prev = k;
    }
  }
  __device__ __forceinline__ void emit(uint64_t i, uint32_t flag, uint32_t prefix) const {
    if (flag) {
      terms[prefix] = key[i];
      list_off[prefix] = i;
    }
  }
};

template <typename SRC>
__global__ void __launch_bounds__(INVB_THREADS) invb_scan_sums_kernel(const SRC src, uint64_t n, uint32_t *sums) {
  __shared__ uint32_t wsum[INVB_THREADS / 64];
  const uint64_t c0 = (uint64_t)blockIdx.x * INVB_SCAN_CHUNK + threadIdx.x * 4;
  uint32_t s = 0;
#pragma unroll
  for (uint32_t r = 0; r < INVB_SCAN_ROUNDS; ++r) {
    uint32_t v[4];
    src.load4(c0 + (uint64_t)r * INVB_THREADS * 4, n, v);
    s += v[0] + v[1] + v[2] + v[3];
  }
  uint32_t total;
  (void)invb_block_scan(s, wsum, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one work-group: sums[] -> its exclusive scan, *total = the sum of everything
__global__ void __launch_bounds__(INVB_THREADS) invb_scan_top_kernel(uint32_t *sums, uint32_t nsums, uint32_t *total) {
  __shared__ uint32_t wsum[INVB_THREADS / 64];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < nsums; b += INVB_THREADS) {                   // (uniform)
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < nsums ? sums[i] : 0u;
    uint32_t tot;
    const uint32_t ex = invb_block_scan(v, wsum, tot);
    if (i < nsums) sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

template <typename SRC>
__global__ void __launch_bounds__(INVB_THREADS) invb_scan_chunks_kernel(const SRC src, uint64_t n, const uint32_t *sums) {
  __shared__ uint32_t wsum[INVB_THREADS / 64];
  uint32_t carry = sums[blockIdx.x];
#pragma unroll
  for (uint32_t r = 0; r < INVB_SCAN_ROUNDS; ++r) {
    const uint64_t i = (uint64_t)blockIdx.x * INVB_SCAN_CHUNK + (uint64_t)r * INVB_THREADS * 4 + threadIdx.x * 4;
    uint32_t v[4];
    src.load4(i, n, v);
    uint32_t tot;
    uint32_t p = carry + invb_block_scan(v[0] + v[1] + v[2] + v[3], wsum, tot);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i + e < n) src.emit(i + e, v[e], p);
      p += v[e];
    }
    carry += tot;
  }
}

// ---- positions and postings -----------------------------------------------------------------------------------------------------
// pos[e] = the row that holds element e; a wave per row, the waves stride over the rows
__global__ void __launch_bounds__(INVB_THREADS) invb_expand_kernel(const uint64_t *row_off, uint64_t n, uint64_t elems, uint32_t *pos) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nwaves = (uint64_t)gridDim.x * (INVB_THREADS / 64);
  for (uint64_t r = (uint64_t)blockIdx.x * (INVB_THREADS / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
    const uint64_t b = row_off[r], e = min(row_off[r + 1], elems);
    for (uint64_t p = b + lane; p < e; p += 64) pos[p] = (uint32_t)r;
  }
}

// WT: the stored value as a word of its width.  ord == nullptr: the elements are in sorted order as they stand.
template <typename WT>
__global__ void __launch_bounds__(INVB_THREADS) invb_gather_kernel(const uint32_t *ord, const uint32_t *pos, const WT *val, uint64_t elems,
                                                                   uint32_t *ppos, WT *pval) {
  const uint64_t i = (uint64_t)blockIdx.x * INVB_THREADS + threadIdx.x;
  if (i >= elems) return;
  const uint64_t o = ord ? ord[i] : i;
  if (o >= elems) return;                                                // (never: the ordinals are a permutation)
  ppos[i] = pos[o];
  pval[i] = val[o];
}

}  // namespace zvk
