// sparse_put_plan.h — the host's share of add-with-id on a sparse index, for both entries (zvec_hip_sparse_put, zvec_hip_sparse_put_dev):
// which rows of a call remain, what they make of the store, where the tables of the call lie in its device workspace, and what the
// call does to the hole bits.  Nothing of HIP: tests/cpp/test_sparse_put_plan_cpu.cc.
//
// FlatSparseStreamerEntity::add_vector_with_id (flat_sparse_streamer_entity.cc:708-783) row by row: id == count appends, id > count
// pads [count, id) with empty rows under kInvalidKey first, id < count overwrites.  Applied in call order that leaves, for every
// position, the LAST row the call names for it, a hole where a gap was padded and never named, and everything else as it was; so the
// call is reduced to its rows sorted by id, the last of every id (put_keep), and applied at once by one of three routes (put_plan):
//   0 tail      every id is at or behind the old count: the append path plus empty rows for the gaps
//   1 in place  every overwritten row keeps its length: pairs and keys are written over the old ones (tail rows, if any, as route 0)
//   2 splice    an overwritten row changes its length: new idx / val / row_off / keys arrays are written whole by one pass over the
//               store and take the old ones' place
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/zvec_hip.h"      // (the error codes)
#include "hole_bits.h"

// The rows that remain: the last one of every id, ascending by id (keep[j] = its number in the call).  n > 0.
inline int put_keep(const uint32_t *ids, uint64_t n, std::vector<uint32_t> &keep) {
  bool ascending = true;
  for (uint64_t i = 0; i < n; ++i) {
    if (ids[i] == 0xffffffffu) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (kInvalidNodeId)
    if (i && ids[i] <= ids[i - 1]) ascending = false;
  }
  keep.resize((size_t)n);
  for (uint64_t i = 0; i < n; ++i) keep[i] = (uint32_t)i;
  if (ascending) return 0;
  std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
  size_t o = 0;
  for (size_t i = 0; i < keep.size(); ++i)
    if (i + 1 == keep.size() || ids[keep[i + 1]] != ids[keep[i]]) keep[o++] = keep[i];      // (stable: the last of a run is the latest)
  keep.resize(o);
  return 0;
}

// The device workspace of a call, in 8-byte words from its start, every part on a 16-byte boundary:
//   tid[T] u32 | src[T] u32 | tval[T] | sb[T + 1] | tkey[T] | tbeg[m] | ds[2m + 3] | ss[2m + 2] | stage idx[S] u32 | stage val[S]
// The first four parts are the plan's tables and need T alone (they end where tkey begins); the rest is placed once m and S are known.
struct SparsePutLayout {
  uint64_t tid = 0, src = 0, tval = 0, sb = 0, tkey = 0, tbeg = 0, ds = 0, ss = 0, sidx = 0, sval = 0, words = 0;
  static uint64_t even(uint64_t w) { return (w + 1) & ~1ull; }
  explicit SparsePutLayout(uint32_t T) {
    src = tid + even(((uint64_t)T + 1) / 2);
    tval = src + even(((uint64_t)T + 1) / 2);
    sb = tval + even(T);
    tkey = sb + even((uint64_t)T + 1);
    tbeg = tkey + even(T);
  }
  void place(uint32_t m, uint64_t S, uint32_t width) {
    ds = tbeg + even(m);
    ss = ds + even(2ull * m + 3);
    sidx = ss + even(2ull * m + 2);
    sval = sidx + even((S + 1) / 2);
    words = sval + even((S * width + 7) / 8);
  }
};

// What a call makes of a store of old_n rows and old_elems pairs.
struct SparsePutPlan {
  uint64_t old_n = 0, old_elems = 0;
  uint32_t T = 0, m = 0;            // kept rows; the first m of them lie below old_n (overwritten), the rest at or behind it (tail)
  uint64_t new_n = 0, new_elems = 0;
  uint64_t S = 0, S_over = 0;       // pairs of the kept rows, the length of the stage; of them the overwritten rows', in front
  uint64_t tail_base = 0;           // where the old rows' pairs end in the new arrays, and the tail rows' begin
  uint64_t gap = 0;                 // holes the call leaves behind the old rows
  bool same = true;                 // every overwritten row keeps its length
  int route = 0;
};

// The plan of a call from its kept rows, and the four tables the device reads it from, written where the caller keeps the
// workspace's words (`ws`, laid out by L: its first L.tkey words):
//   tid[j]   the id of kept row j          src[j]   its number in the call (keep[j])
//   sb[j]    where its pairs begin in the stage, sb[T] = S
//   tval[j]  for an overwritten row the new minus the old pairs of the overwritten rows up to and including it; for a tail row the
//            offset its pairs end at (SparsePutOffsetsArgs, zvk_sparse_put.hip.h)
// old_len[i]: the pairs stored now at the id of the CALL's row i; read for overwritten rows only (may be NULL when there is none).
// max_count: the pairs a stored row can have; chunk: destination elements per work-group of the splice.  Refused here: a row count
// or a splice grid beyond 32 bits, and an old length no sound store has.
inline int put_plan(SparsePutPlan &p, const std::vector<uint32_t> &keep, const uint32_t *ids, const uint32_t *counts, const uint32_t *old_len,
                    uint64_t old_n, uint64_t old_elems, uint32_t max_count, uint32_t chunk, const SparsePutLayout &L, uint64_t *ws) {
  p = SparsePutPlan();
  p.old_n = old_n; p.old_elems = old_elems;
  p.T = (uint32_t)keep.size();
  p.new_n = std::max<uint64_t>(old_n, (uint64_t)ids[keep.back()] + 1);
  if (p.new_n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (positions are 32-bit in the partial lists, as in append)
  while (p.m < p.T && ids[keep[p.m]] < old_n) ++p.m;
  uint32_t *tid = reinterpret_cast<uint32_t *>(ws + L.tid), *src = reinterpret_cast<uint32_t *>(ws + L.src);
  int64_t *tval = reinterpret_cast<int64_t *>(ws + L.tval);
  uint64_t *sb = ws + L.sb;
  int64_t shift = 0;
  sb[0] = 0;
  for (uint32_t j = 0; j < p.T; ++j) {
    tid[j] = ids[keep[j]];
    src[j] = keep[j];
    sb[j + 1] = sb[j] + counts[keep[j]];
    if (j < p.m) {
      const uint64_t nl = counts[keep[j]], ol = old_len[keep[j]];
      if (ol > max_count) return ZVEC_HIP_ERR_RUNTIME;               // (the store's own offsets: never)
      p.same = p.same && nl == ol;
      shift += (int64_t)nl - (int64_t)ol;
      tval[j] = shift;
    }
  }
  p.S = sb[p.T];
  p.S_over = sb[p.m];
  p.tail_base = old_elems + (uint64_t)shift;
  p.new_elems = p.tail_base + (p.S - p.S_over);
  for (uint32_t j = p.m; j < p.T; ++j) tval[j] = (int64_t)(p.tail_base + (sb[j + 1] - p.S_over));
  p.route = p.m == 0 ? 0 : p.same ? 1 : 2;
  p.gap = (p.new_n - old_n) - (p.T - p.m);
  if (p.route == 2 && (p.new_elems + chunk - 1) / chunk > 0x7fffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (the splice's grid)
  return 0;
}

// The hole bits after the call (they span new_n positions already): the gaps between the old end and the call's tail rows are set, a
// written hole is cleared (no gap, no hole: no pass).  tid: the plan's table.
inline void put_holes(HoleWords &holes, const SparsePutPlan &p, const uint32_t *tid) {
  uint64_t from = p.old_n;
  for (uint32_t j = p.m; j < p.T && p.gap; ++j) { holes.set_range(from, tid[j]); from = (uint64_t)tid[j] + 1; }
  for (uint32_t j = 0; j < p.m && holes.nholes; ++j) holes.clear(tid[j]);
}
