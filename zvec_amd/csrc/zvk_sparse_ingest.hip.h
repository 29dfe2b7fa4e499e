// zvk_sparse_ingest.hip.h — rows of a sparse index that are already in device memory: dense matrices -> CSR, and the checks of CSR
// that arrives on the device (zvec_hip_sparse_append_dev / _append_dense_dev / _from_dense_dev / _search_dense_dev).
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// A dense row is cut into SLICES of SPARSE_INGEST_SLICE columns; a work item is (row, slice) and belongs to one wave, the waves
// stride over the items.  So one query of 30 522 columns is 30 items and a matrix of many rows is simply more of them: the grid
// covers the device whether the call is narrow or tall.  Three steps, the matrix is read twice and nothing else is:
//   sparse_dense_count_kernel   kept elements of every item -> item_cnt[]
//   the exclusive scan of zvk_sparse_invb.hip.h over item_cnt[] (IngestCounts: 32-bit prefixes inside a segment of at most 2^20
//                               items, on top of the 64-bit sum of the segments before it) -> item_off[]; the last one is the total
//   sparse_ingest_rows_kernel   a row's count = the distance of its first slice's offset to the next row's; a row above the cap
//                               sets ST_LONG in the status word
//   sparse_dense_fill_kernel    the same walk; every kept element goes to item_off[item] + its rank among the item's kept ones
// An element is KEPT iff its bits without the sign are not zero: +0 and -0 go, subnormals, inf and NaN stay, and the value is
// written as it is read (a word of the value's width, never converted).  The rank is the number of kept elements in front of the
// element in column order — ballots of "kept" and the popcount of the lower lanes —, so a run ascends strictly by construction and
// the same matrix gives the same bytes every time; no atomic decides where anything lands.
//
// Alignment.  Neither the base pointer nor ld * sizeof(value) needs to be a multiple of 16: a slice is walked as a head of single
// elements up to the first 16-byte boundary, whole 16-byte vectors (a lane takes 4 fp32 or 8 fp16 columns, 1 KiB a wave and
// step), and a tail of single elements.  Nothing outside [row + slice begin, row + slice end) is read.  The pointer must be a
// multiple of the value's own width (the host refuses anything else).
//
// CSR from the device: the same scan over the caller's counts (each clamped to cap + 1 so that a segment's sum stays 32-bit: a
// count above the cap is refused anyway), then sparse_csr_check_kernel, a wave per row: count <= cap, the run inside
// [0, elements), every index above its predecessor.  The host compares the scan's total with `elements`.
#pragma once
#include "zvk_common.hip.h"
#include "zvk_sparse.hip.h"
#include "zvk_sparse_invb.hip.h"

namespace zvk {

constexpr uint32_t SPARSE_INGEST_SLICE = 1024;         // columns of one work item (slice_cols)
constexpr uint32_t SPARSE_INGEST_THREADS = 256;        // 4 waves
constexpr uint64_t SPARSE_INGEST_SEG = 1ull << 20;     // items of one scan segment: 2^20 * (4096 + 1) < 2^32
// the status word
constexpr uint32_t SPARSE_INGEST_ST_LONG = 1u;         // a row above the cap
constexpr uint32_t SPARSE_INGEST_ST_ORDER = 2u;        // an index not above its predecessor
constexpr uint32_t SPARSE_INGEST_ST_SUM = 4u;          // a run that leaves [0, elements)

// the scan's source: item counts in, 64-bit offsets out (zvk_sparse_invb.hip.h, invb_scan_*_kernel)
struct IngestCounts {
  const uint32_t *cnt;                   // [n] of this segment
  uint64_t *off;                         // [n]
  const uint64_t *base;                  // the sum of the segments in front
  uint32_t clamp;
  __device__ __forceinline__ void load4(uint64_t i, uint64_t n, uint32_t v[4]) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? min(cnt[i + e], clamp) : 0u;
  }
  __device__ __forceinline__ void emit(uint64_t i, uint32_t, uint32_t prefix) const { off[i] = *base + prefix; }
};

// after a segment's scan: acc[seg + 1] = acc[seg] + the segment's sum; it is also the offset behind the segment's last item
// and, after the last segment, the total
__global__ void sparse_ingest_seg_kernel(uint64_t *acc, uint32_t seg, const uint32_t *seg_sum, uint64_t *off_end, uint64_t *total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint64_t t = acc[seg] + *seg_sum;
    acc[seg + 1] = t;
    *off_end = t;
    *total = t;
  }
}

template <typename WT>
__device__ __forceinline__ bool ingest_kept(WT bits) { return (WT)(bits << 1) != 0; }

// One slice: `len` columns at p, the first of them column col0.  Returns the kept elements (the same in every lane).  FILL: the
// kept ones go to oi[] / ov[] in column order, at most `room` of them (the count pass said how many: a matrix that changed
// since then loses elements instead of writing past its item).
template <typename WT, bool FILL>
__device__ __forceinline__ uint32_t ingest_walk(const WT *p, uint32_t len, uint32_t col0, uint32_t lane, uint32_t *oi, WT *ov,
                                                uint64_t room) {
  constexpr uint32_t V = 16 / sizeof(WT);
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t run = 0;
  auto singles = [&](uint32_t e0, uint32_t cnt) {      // (cnt < V)
    const bool in = lane < cnt;
    const WT w = in ? p[e0 + lane] : (WT)0;
    const bool k = in && ingest_kept(w);
    const uint64_t m = __ballot(k);
    if (FILL && k) {
      const uint32_t pos = run + (uint32_t)__popcll(m & below);
      if (pos < room) { oi[pos] = col0 + e0 + lane; ov[pos] = w; }
    }
    run += (uint32_t)__popcll(m);
  };
  const uint32_t head = min(len, (uint32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(WT)));
  if (head) singles(0, head);
  const uint32_t nvec = (len - head) / V;
  const u32x4 *vp = reinterpret_cast<const u32x4 *>(p + head);
  for (uint32_t vb = 0; vb < nvec; vb += 64) {         // (uniform)
    const uint32_t v = vb + lane;
    u32x4 x = {0u, 0u, 0u, 0u};
    if (v < nvec) x = vp[v];
    WT w[V];
#pragma unroll
    for (uint32_t j = 0; j < V; ++j) {
      if constexpr (sizeof(WT) == 4) w[j] = x[j];
      else w[j] = (WT)(x[j / 2] >> (16 * (j & 1)));
    }
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t j = 0; j < V; ++j) {
      const uint64_t m = __ballot(ingest_kept(w[j]));  // (a lane behind the last vector holds zeros)
      before += (uint32_t)__popcll(m & below);
      tot += (uint32_t)__popcll(m);
    }
    if (FILL) {
      uint32_t pos = run + before;                     // the lanes below come first, then this lane's own columns in order
#pragma unroll
      for (uint32_t j = 0; j < V; ++j) {
        if (ingest_kept(w[j])) {
          if (pos < room) { oi[pos] = col0 + head + v * V + j; ov[pos] = w[j]; }
          ++pos;
        }
      }
    }
    run += tot;
  }
  const uint32_t done = head + nvec * V;
  if (done < len) singles(done, len - done);
  return run;
}

// rows: [n] rows of `dim` columns, `ld` elements apart; nsl = slices of a row (at least 1: dim == 0 gives one empty slice)
template <typename WT>
__global__ void __launch_bounds__(SPARSE_INGEST_THREADS) sparse_dense_count_kernel(const WT *rows, uint64_t n, uint32_t dim, uint64_t ld,
                                                                                   uint32_t nsl, uint32_t *item_cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nitems = n * nsl, nwaves = (uint64_t)gridDim.x * (SPARSE_INGEST_THREADS / 64);
  for (uint64_t i = (uint64_t)blockIdx.x * (SPARSE_INGEST_THREADS / 64) + (threadIdx.x >> 6); i < nitems; i += nwaves) {
    const uint64_t r = i / nsl;
    const uint32_t c0 = (uint32_t)(i % nsl) * SPARSE_INGEST_SLICE;
    const uint32_t len = c0 < dim ? min(SPARSE_INGEST_SLICE, dim - c0) : 0u;
    const uint32_t c = ingest_walk<WT, false>(rows + r * ld + c0, len, c0, lane, nullptr, nullptr, 0);
    if (lane == 0) item_cnt[i] = c;
  }
}

// item_off: [nitems + 1]; the pairs of item i go to out_idx / out_val [item_off[i], item_off[i + 1])
template <typename WT>
__global__ void __launch_bounds__(SPARSE_INGEST_THREADS) sparse_dense_fill_kernel(const WT *rows, uint64_t n, uint32_t dim, uint64_t ld,
                                                                                  uint32_t nsl, const uint64_t *item_off, uint32_t *out_idx,
                                                                                  WT *out_val) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nitems = n * nsl, nwaves = (uint64_t)gridDim.x * (SPARSE_INGEST_THREADS / 64);
  for (uint64_t i = (uint64_t)blockIdx.x * (SPARSE_INGEST_THREADS / 64) + (threadIdx.x >> 6); i < nitems; i += nwaves) {
    const uint64_t r = i / nsl;
    const uint32_t c0 = (uint32_t)(i % nsl) * SPARSE_INGEST_SLICE;
    const uint32_t len = c0 < dim ? min(SPARSE_INGEST_SLICE, dim - c0) : 0u;
    const uint64_t b = item_off[i], e = item_off[i + 1];
    if (e <= b) continue;                                // (uniform: nothing kept)
    (void)ingest_walk<WT, true>(rows + r * ld + c0, len, c0, lane, out_idx + b, out_val + b, e - b);
  }
}

// off: [n * stride + 1] offsets, row r begins at off[r * stride].  counts (nullable): the rows' lengths.  A row above `cap` sets
// ST_LONG (an ordinary atomic OR: the same word in any order).
__global__ void __launch_bounds__(SPARSE_INGEST_THREADS) sparse_ingest_rows_kernel(const uint64_t *off, uint32_t stride, uint64_t n,
                                                                                   uint32_t cap, uint32_t *counts, uint32_t *status) {
  const uint64_t r = (uint64_t)blockIdx.x * SPARSE_INGEST_THREADS + threadIdx.x;
  if (r >= n) return;
  const uint64_t c = off[(r + 1) * stride] - off[r * stride];
  if (counts) counts[r] = (uint32_t)c;                   // (at most the row's columns)
  if (c > cap) atomicOr(status, SPARSE_INGEST_ST_LONG);
}

// The rows' place in the store: row_off[row0 + 1 + r] = elems0 + off[(r + 1) * stride], keys[row0 + r] = d_keys[r], or the
// storage position where there are none.
__global__ void __launch_bounds__(SPARSE_INGEST_THREADS) sparse_ingest_commit_kernel(const uint64_t *off, uint32_t stride, uint64_t n,
                                                                                     uint64_t elems0, uint64_t row0, const uint64_t *d_keys,
                                                                                     uint64_t *row_off, uint64_t *keys) {
  const uint64_t r = (uint64_t)blockIdx.x * SPARSE_INGEST_THREADS + threadIdx.x;
  if (r >= n) return;
  row_off[row0 + 1 + r] = elems0 + off[(r + 1) * stride];
  keys[row0 + r] = d_keys ? d_keys[r] : row0 + r;
}

// CSR as the caller left it on the device: counts[n], off[n] from the scan of the clamped counts, idx[elements].  A wave per row.
__global__ void __launch_bounds__(SPARSE_INGEST_THREADS) sparse_csr_check_kernel(const uint32_t *counts, const uint32_t *idx,
                                                                                 const uint64_t *off, uint64_t n, uint64_t elements,
                                                                                 uint32_t *status) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nwaves = (uint64_t)gridDim.x * (SPARSE_INGEST_THREADS / 64);
  uint32_t bad = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (SPARSE_INGEST_THREADS / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
    const uint32_t c = counts[r];
    if (c > SPARSE_MAX_COUNT) { bad |= SPARSE_INGEST_ST_LONG; continue; }
    const uint64_t b = off[r];
    if (b + c > elements) { bad |= SPARSE_INGEST_ST_SUM; continue; }      // (never read outside idx[0, elements))
    for (uint32_t e = 1 + lane; e < c; e += 64)
      if (idx[b + e] <= idx[b + e - 1]) bad |= SPARSE_INGEST_ST_ORDER;
  }
  if (bad) atomicOr(status, bad);
}

}  // namespace zvk
