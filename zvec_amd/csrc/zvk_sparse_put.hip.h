// zvk_sparse_put.hip.h — add-with-id on a sparse index (zvec_hip_sparse_put / _put_dev): the device side of the three routes.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// The store is a packed CSR (row_off[n + 1], idx, val, keys) and every scoring kernel relies on row_off[r] .. row_off[r + 1] being
// the row, so a row that changes its length moves everything behind it.  The host (host/sparse_put_plan.h) sorts the rows of a
// call by id, keeps the last one of every id and plans where their pairs lie back to back ("the stage").  The
// kernels, the same for both entries (the first is launched by the entry, the others by put_apply, api_entry_sparse_put.inc.h):
//
//   sparse_put_lens_kernel      before the plan: the old lengths at the call's ids (4 bytes a row: the host learns them from the
//                               device and keeps no mirror of row_off)
//   sparse_put_pieces_kernel    for overwritten rows: where each begins (tbeg) and the piece table of the splice (ds, ss), from the
//                               store's own offsets and the plan's shifts
//   sparse_put_rows_kernel      route 1: every overwritten row keeps its length -> its pairs and its key are written over the old
//                               ones, a work-group per row
//   sparse_put_splice_kernel    route 2: the new idx / val arrays whole, out of place.  The overwritten rows cut the old arrays into
//                               untouched segments; in the new arrays the pieces alternate: segment 0, new row 0, segment 1, ...,
//                               segment m, the call's tail rows.  Even pieces read the old arrays, odd ones the stage, each at a
//                               constant shift.  A work-group takes SPARSE_PUT_CHUNK consecutive destination elements, finds its
//                               first piece by a search in ds[] and walks the pieces that reach into its chunk.
//   sparse_put_offsets_kernel   row_off and keys of the positions [r0, new_n): old offset + the shift behind the overwritten rows at
//                               or below the position, the tail rows' ends, the invalid key for a hole.  Route 2 runs it over every
//                               position into new arrays; routes 0 and 1 over the call's tail in place.
//
// zvec_hip_sparse_put stages the pairs and the keys on the host and uploads them; zvec_hip_sparse_put_dev (the call's rows in device
// memory) makes them on the device from the plan's tables: sparse_put_stage_kernel at the end of this file.
//
// Values are moved as bits.  Halves (fp16) are moved as 32-bit words wherever the destination allows it: a piece that starts or ends
// in the middle of a destination word writes that half alone (the other half belongs to the neighbouring piece, possibly to another
// work-group: the two never write the same bytes), and a piece whose shift is odd reads its source one half off the word grid, which
// the copy below puts together from aligned words and the two halves at its ends.  Nothing is read outside the piece's source range.
#pragma once
#include "zvk_common.hip.h"
#include "zvk_sparse_invb.hip.h"      // u32x4

namespace zvk {

constexpr uint32_t SPARSE_PUT_THREADS = 256;
constexpr uint32_t SPARSE_PUT_CHUNK = 4096;      // destination elements per work-group of the splice (chunk_elems); a multiple of 8

// dst[e] = src[e + delta] for e in [a, b), 32-bit words, by the whole work-group: 16-byte stores on the destination's grid, 16-byte
// loads where the shift keeps the source on it.  Both arrays start on a 16-byte boundary.
__device__ __forceinline__ void put_copy_words(uint32_t *dst, const uint32_t *src, uint64_t a, uint64_t b, int64_t delta) {
  const uint32_t t = threadIdx.x;
  const uint64_t a4 = min(b, (a + 3) & ~3ull), b4 = max(a4, b & ~3ull);
  if (a + t < a4) dst[a + t] = src[(int64_t)(a + t) + delta];
  if (b4 + t < b) dst[b4 + t] = src[(int64_t)(b4 + t) + delta];
  const bool aligned = (delta & 3) == 0;
  for (uint64_t e = a4 + 4ull * t; e < b4; e += 4ull * SPARSE_PUT_THREADS) {
    const uint32_t *s = src + ((int64_t)e + delta);
    u32x4 v;
    if (aligned) {
      v = *reinterpret_cast<const u32x4 *>(s);
    } else {
      v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
    }
    *reinterpret_cast<u32x4 *>(dst + e) = v;
  }
}

// the same for 16-bit elements, [a, b) and delta in elements
__device__ __forceinline__ void put_copy_halves(uint16_t *dst, const uint16_t *src, uint64_t a, uint64_t b, int64_t delta) {
  const uint32_t t = threadIdx.x;
  if (a >= b) return;
  if (a & 1) {                                    // the piece starts in the middle of a destination word
    if (t == 0) dst[a] = src[(int64_t)a + delta];
    ++a;
  }
  if (b > a && (b & 1)) {                         // ... or ends in one
    --b;
    if (t == 0) dst[b] = src[(int64_t)b + delta];
  }
  if (a >= b) return;
  uint32_t *dw = reinterpret_cast<uint32_t *>(dst);
  if ((delta & 1) == 0) {                         // source and destination agree in 4-byte alignment
    put_copy_words(dw, reinterpret_cast<const uint32_t *>(src), a >> 1, b >> 1, delta / 2);
    return;
  }
  // odd shift: destination word w = halves src[2w + delta], src[2w + delta + 1], the first one at an odd place.  Four words at a time:
  // the half in front, three aligned words, the half behind (all eight halves are the piece's own); single words at the ends.
  const uint64_t wa = a >> 1, wb = b >> 1;
  const uint64_t w4 = min(wb, (wa + 3) & ~3ull), e4 = max(w4, wb & ~3ull);
  auto one = [&](uint64_t w) {
    const uint16_t *s = src + ((int64_t)(2 * w) + delta);
    dw[w] = (uint32_t)s[0] | ((uint32_t)s[1] << 16);
  };
  if (wa + t < w4) one(wa + t);
  if (e4 + t < wb) one(e4 + t);
  for (uint64_t w = w4 + 4ull * t; w < e4; w += 4ull * SPARSE_PUT_THREADS) {
    const uint16_t *s = src + ((int64_t)(2 * w) + delta);
    const uint32_t h0 = s[0], h7 = s[7];
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s + 1);
    const uint32_t w1 = sw[0], w2 = sw[1], w3 = sw[2];
    u32x4 v;
    v.x = h0 | (w1 << 16);
    v.y = (w1 >> 16) | (w2 << 16);
    v.z = (w2 >> 16) | (w3 << 16);
    v.w = (w3 >> 16) | (h7 << 16);
    *reinterpret_cast<u32x4 *>(dw + w) = v;
  }
}

template <typename W>
__device__ __forceinline__ void put_copy_values(void *dst, const void *src, uint64_t a, uint64_t b, int64_t delta) {
  if constexpr (sizeof(W) == 4) put_copy_words(static_cast<uint32_t *>(dst), static_cast<const uint32_t *>(src), a, b, delta);
  else put_copy_halves(static_cast<uint16_t *>(dst), static_cast<const uint16_t *>(src), a, b, delta);
}

// Route 1.  Row j of the m overwritten ones: stage[sbeg[j] .. sbeg[j + 1]) goes to the elements from tbeg[j] on (its old place,
// its old length), its key to keys[tid[j]].
struct SparsePutRowsArgs {
  const uint32_t *tid;
  const uint64_t *tkey, *tbeg, *sbeg;
  const uint32_t *stage_idx;
  const void *stage_val;
  uint32_t *idx;
  void *val;
  uint64_t *keys;
};

template <typename W>
__global__ void __launch_bounds__(SPARSE_PUT_THREADS) sparse_put_rows_kernel(SparsePutRowsArgs a) {
  const uint32_t j = blockIdx.x;
  const uint64_t d0 = a.tbeg[j], s0 = a.sbeg[j], len = a.sbeg[j + 1] - s0;
  const int64_t delta = (int64_t)s0 - (int64_t)d0;
  put_copy_words(a.idx, a.stage_idx, d0, d0 + len, delta);
  put_copy_values<W>(a.val, a.stage_val, d0, d0 + len, delta);
  if (threadIdx.x == 0) a.keys[a.tid[j]] = a.tkey[j];
}

// Route 2.  ds[npieces + 1]: the first destination element of every piece, ascending (an empty piece repeats its successor's),
// ds[0] = 0 and ds[npieces] = elems, the new element count; ss[npieces]: the first source element, in the old arrays for an even
// piece and in the stage for an odd one.  Grid: ceil(elems / SPARSE_PUT_CHUNK).
struct SparsePutSpliceArgs {
  const uint64_t *ds, *ss;
  uint32_t npieces;
  uint64_t elems;
  const uint32_t *old_idx, *stage_idx;
  const void *old_val, *stage_val;
  uint32_t *new_idx;
  void *new_val;
};

template <typename W>
__global__ void __launch_bounds__(SPARSE_PUT_THREADS) sparse_put_splice_kernel(SparsePutSpliceArgs a) {
  const uint64_t c0 = (uint64_t)blockIdx.x * SPARSE_PUT_CHUNK, c1 = min(c0 + SPARSE_PUT_CHUNK, a.elems);
  // the first piece that starts behind c0 (ds[npieces] = elems > c0 does); the one in front of it holds c0
  uint32_t lo = 0, hi = a.npieces;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.ds[mid] <= c0) lo = mid + 1;
    else hi = mid;
  }
  for (uint32_t p = lo - 1; p < a.npieces; ++p) {
    const uint64_t p0 = a.ds[p];
    if (p0 >= c1) break;
    const uint64_t b0 = max(p0, c0), b1 = min(a.ds[p + 1], c1);
    if (b0 >= b1) continue;
    const int64_t delta = (int64_t)a.ss[p] - (int64_t)p0;
    const bool staged = (p & 1u) != 0;
    put_copy_words(a.new_idx, staged ? a.stage_idx : a.old_idx, b0, b1, delta);
    put_copy_values<W>(a.new_val, staged ? a.stage_val : a.old_val, b0, b1, delta);
  }
}

// row_off[r + 1] and keys[r] for r in [r0, new_n).  tid[T]: the call's rows ascending by id, the first m of them below old_n
// (overwritten), the rest at or behind it (tail).  tval[j]: for an overwritten row the new minus the old element count of the
// overwritten rows up to and including it; for a tail row the offset its pairs end at.  tail_base: where the old rows' elements end
// in the new arrays.  A position that is neither old nor named is a hole: an empty row under the invalid key.  old_keys == new_keys
// (in place): the keys of the other old rows are left alone.
struct SparsePutOffsetsArgs {
  const uint32_t *tid;
  const uint64_t *tkey;
  const int64_t *tval;
  uint32_t T, m;
  uint64_t old_n, r0, new_n, tail_base;
  const uint64_t *old_off, *old_keys;
  uint64_t *new_off, *new_keys;
};

__global__ void __launch_bounds__(SPARSE_PUT_THREADS) sparse_put_offsets_kernel(SparsePutOffsetsArgs a) {
  const uint64_t r = a.r0 + (uint64_t)blockIdx.x * SPARSE_PUT_THREADS + threadIdx.x;
  if (r >= a.new_n) return;
  uint32_t lo = 0, hi = a.T;                       // -> the number of the call's rows with id <= r
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)a.tid[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t j = lo;
  uint64_t end;
  if (r < a.old_n) end = a.old_off[r + 1] + (uint64_t)(j ? a.tval[j - 1] : 0);
  else end = j > a.m ? (uint64_t)a.tval[j - 1] : a.tail_base;
  a.new_off[r + 1] = end;
  if (r == 0) a.new_off[0] = 0;
  if (j && (uint64_t)a.tid[j - 1] == r) a.new_keys[r] = a.tkey[j - 1];
  else if (r >= a.old_n) a.new_keys[r] = ~0ull;                        // kInvalidKey
  else if (a.new_keys != a.old_keys) a.new_keys[r] = a.old_keys[r];
}

// ---- what the plan is made from, and what is made from the plan ------------------------------------------------------------------

// len[i] = the pairs stored at position ids[i] now, 0 for an id at or behind the count
__global__ void sparse_put_lens_kernel(const uint64_t *row_off, const uint32_t *ids, uint64_t n, uint64_t old_n, uint32_t *len) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t id = ids[i];
  len[i] = id < old_n ? (uint32_t)(row_off[id + 1] - row_off[id]) : 0u;      // (a stored row has at most 4096 pairs)
}

// tbeg[m], ds[2m + 3] and ss[2m + 2] as SparsePutRowsArgs / SparsePutSpliceArgs describe them, from the store's own offsets.
// tid[m]: the overwritten rows ascending; tval[j]: the new minus the old pairs of the overwritten rows up to and including j;
// sb[m + 1]: where they begin in the stage.  Thread j <= m writes the untouched segment in front of row j and row j itself; the
// last one the segment behind the last row, the call's tail rows and the end.  (m > 0)
struct SparsePutPiecesArgs {
  const uint64_t *row_off;
  const uint32_t *tid;
  const int64_t *tval;
  const uint64_t *sb;
  uint32_t m;
  uint64_t tail_base, new_elems;
  uint64_t *tbeg, *ds, *ss;
};

__global__ void __launch_bounds__(SPARSE_PUT_THREADS) sparse_put_pieces_kernel(SparsePutPiecesArgs a) {
  const uint32_t j = blockIdx.x * SPARSE_PUT_THREADS + threadIdx.x;
  if (j > a.m) return;
  const uint64_t prev_end = j ? a.row_off[(uint64_t)a.tid[j - 1] + 1] : 0;
  const uint64_t shift = j ? (uint64_t)a.tval[j - 1] : 0;
  a.ds[2 * (size_t)j] = prev_end + shift;
  a.ss[2 * (size_t)j] = prev_end;
  if (j < a.m) {
    const uint64_t ob = a.row_off[a.tid[j]];
    a.ds[2 * (size_t)j + 1] = ob + shift;
    a.ss[2 * (size_t)j + 1] = a.sb[j];
    a.tbeg[j] = ob;
  } else {
    a.ds[2 * (size_t)j + 1] = a.tail_base;
    a.ss[2 * (size_t)j + 1] = a.sb[j];
    a.ds[2 * (size_t)j + 2] = a.new_elems;
  }
}

// The call's rows already in device memory (zvec_hip_sparse_put_dev): the pairs never leave the device, and this kernel builds from
// the plan's tables what the host put uploads, the stage and the keys of the kept rows.
// The stage gather.  Kept row j (ascending by id) is row src[j] of the call: its pairs, in_idx / in_val [in_off[src[j]], + len),
// len = sb[j + 1] - sb[j], go to the stage from element sb[j] on, and its key (the caller's, or the id) to tkey[j].  A wave per row,
// the waves stride over the rows, lane = pair.  The caller's arrays are aligned to their element only.  Indices and fp32 values move
// as words.  Halves: the stage is word-aligned at even elements, so a row that begins at an odd one writes that half alone, and one
// that ends at an odd one its last half; the words between are copied as words where the source run lies on the same parity, and are
// put together from two halves where it does not.  A word of the stage that two rows share is written by each as its own half:
// no two lanes write the same bytes, and nothing outside a row's source run is read.  Rows the keep-last rule dropped are not in src.
struct SparsePutStageArgs {
  const uint32_t *src, *tid;       // [T]
  const uint64_t *sb;              // [T + 1]
  const uint64_t *in_off;          // [n]: where the call's runs begin (the scan of its counts)
  const uint32_t *in_idx;
  const void *in_val;
  const uint64_t *in_keys;         // [n] or NULL
  uint32_t T;
  uint32_t *stage_idx;
  void *stage_val;
  uint64_t *tkey;                  // [T]
};

template <typename W>
__global__ void __launch_bounds__(SPARSE_PUT_THREADS) sparse_put_stage_kernel(SparsePutStageArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nwaves = gridDim.x * (SPARSE_PUT_THREADS / 64);
  for (uint32_t j = blockIdx.x * (SPARSE_PUT_THREADS / 64) + (threadIdx.x >> 6); j < a.T; j += nwaves) {
    const uint32_t r = a.src[j];
    const uint64_t d0 = a.sb[j];
    const uint32_t len = (uint32_t)(a.sb[j + 1] - d0);
    if (lane == 0) a.tkey[j] = a.in_keys ? a.in_keys[r] : (uint64_t)a.tid[j];
    if (len == 0) continue;                              // (uniform; in_off[r] may be the arrays' end)
    const uint64_t s0 = a.in_off[r];
    const uint32_t *si = a.in_idx + s0;
    uint32_t *di = a.stage_idx + d0;
    for (uint32_t e = lane; e < len; e += 64) di[e] = si[e];
    if constexpr (sizeof(W) == 4) {
      const uint32_t *sv = static_cast<const uint32_t *>(a.in_val) + s0;
      uint32_t *dv = static_cast<uint32_t *>(a.stage_val) + d0;
      for (uint32_t e = lane; e < len; e += 64) dv[e] = sv[e];
    } else {
      const uint16_t *sv = static_cast<const uint16_t *>(a.in_val) + s0;
      uint16_t *dv = static_cast<uint16_t *>(a.stage_val) + d0;
      const uint32_t head = (uint32_t)(d0 & 1);                        // halves in front of the first whole word of the stage
      const uint32_t nw = (len - head) / 2;                            // whole words
      const uint32_t done = head + 2 * nw;
      if (lane == 0 && head) dv[0] = sv[0];
      if (lane == 1 && done < len) dv[done] = sv[done];
      uint32_t *dw = reinterpret_cast<uint32_t *>(dv + head);
      const uint16_t *sh = sv + head;
      if ((reinterpret_cast<uintptr_t>(sh) & 2u) == 0) {               // the same parity: words from words
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(sh);
        for (uint32_t w = lane; w < nw; w += 64) dw[w] = sw[w];
      } else {
        for (uint32_t w = lane; w < nw; w += 64) dw[w] = (uint32_t)sh[2 * w] | ((uint32_t)sh[2 * w + 1] << 16);
      }
    }
  }
}

}  // namespace zvk
