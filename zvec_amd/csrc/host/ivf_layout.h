// ivf_layout.h — the host's share of an IVF index's build: which shard owns which inverted list, where every list lies in the blocked
// store, where the next row of a streamed fill goes, and the deal order of the scan's work queue.  Nothing of HIP:
// tests/cpp/test_ivf_layout_cpu.cc.
//
// A list occupies whole 128-row tiles of the store (IVFDumper lays lists out block by block, ivf_dumper.h:33-160: every list's extent
// is known before its blocks are written).  begin() lays out the lists this shard owns from the GLOBAL list sizes, place() plans one
// chunk of rows of a fill (all of it or nothing), finish() closes a complete fill.  A refused call has changed nothing.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../../include/zvec_hip.h"      // (the error codes)

constexpr uint32_t IVF_TILE_ROWS = 128;

// tiles a list of `size` rows occupies: the one place the round-up is written
inline uint64_t ivf_tiles(uint64_t size) { return (size + IVF_TILE_ROWS - 1) / IVF_TILE_ROWS; }

// Greedy largest-first (LPT) assignment of inverted lists to shards, weighted by the 128-row tiles a list occupies in
// HBM (= the bytes a scan streams).  Deterministic: lists ordered by (tiles desc, list id asc), each given to the shard
// with the least tiles so far (lowest shard id on ties) — every rank computes the same map from the global list sizes.
// "whole inverted lists assigned to GPUs (balanced by bytes, list->GPU map)".
inline void ivf_lpt_owner(const uint32_t *sizes, uint32_t nlist, uint32_t nshards, uint32_t *owner, uint64_t *rows_out) {
  std::vector<uint64_t> load(nshards, 0), rows(nshards, 0);
  if (nshards <= 1) {
    for (uint32_t l = 0; l < nlist; ++l) { owner[l] = 0; rows[0] += sizes[l]; }
  } else {
    std::vector<uint32_t> order(nlist);
    for (uint32_t l = 0; l < nlist; ++l) order[l] = l;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return sizes[x] > sizes[y]; });
    for (uint32_t i = 0; i < nlist; ++i) {
      const uint32_t l = order[i];
      uint32_t best = 0;
      for (uint32_t g = 1; g < nshards; ++g)
        if (load[g] < load[best]) best = g;
      owner[l] = best;
      load[best] += ivf_tiles(sizes[l]);
      rows[best] += sizes[l];
    }
  }
  if (rows_out) for (uint32_t g = 0; g < nshards; ++g) rows_out[g] = rows[g];
}

struct IvfLayout {
  uint32_t nlist = 0;                  // lists (= centroids; set with the centroids, before any list is laid out)
  uint32_t shard = 0, nshards = 1;     // the lists kept: those the map gives `shard` of `nshards`
  std::vector<uint32_t> owner;         // list -> shard (byte-balanced, identical on every rank)
  std::vector<uint32_t> size, size_global, tile0;      // rows held here | rows of the whole index | first tile, per list
  std::vector<uint64_t> dense0;        // local dense offsets (nlist + 1): the lists back to back without padding
  std::vector<uint64_t> cursor;        // streamed fill: next dense position of each list
  std::vector<uint64_t> row_ids;       // local dense position -> original row
  std::vector<uint32_t> order;         // deal order of the scan's work queue: lists largest first
  std::vector<uint32_t> tail;          // level of a list in that order: 0 head (longer chunks), 1, 2 tail (shorter chunks)
  std::vector<uint64_t> rows_of_largest;   // [i] = rows of the i largest local lists (bound of what i probes can scan)
  uint64_t count_local = 0, count_global = 0;
  uint64_t local_tiles = 0;            // tiles of the lists held by this shard
  uint32_t tiles_per_chunk = 8;

  // Lay out the owned lists and reset the cursors.  Positions are 32-bit: a shard of 0xffffffff padded rows or more is refused before
  // anything is allocated per row and before any member changes.
  int begin(const uint32_t *sizes_global, uint32_t nlist_) {
    std::vector<uint32_t> own(nlist_, 0), sz(nlist_, 0), t0(nlist_, 0);
    std::vector<uint64_t> d0((size_t)nlist_ + 1, 0);
    ivf_lpt_owner(sizes_global, nlist_, nshards, own.data(), nullptr);
    uint64_t total = 0, tiles = 0, dense = 0;
    for (uint32_t l = 0; l < nlist_; ++l) {
      total += sizes_global[l];
      if (own[l] == shard) sz[l] = sizes_global[l];
      t0[l] = (uint32_t)tiles;
      d0[l] = dense;
      tiles += ivf_tiles(sz[l]);
      dense += sz[l];
    }
    d0[nlist_] = dense;
    if (tiles * IVF_TILE_ROWS >= 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
    std::vector<uint64_t> ids(dense, 0);
    nlist = nlist_;
    size_global.assign(sizes_global, sizes_global + nlist_);
    owner.swap(own); size.swap(sz); tile0.swap(t0); dense0.swap(d0); row_ids.swap(ids);
    cursor.assign(dense0.begin(), dense0.end() - 1);
    count_local = dense; count_global = total; local_tiles = tiles;
    return 0;
  }

  // One chunk of a fill: rows [0, n) of the caller's chunk with their labels; the rows of owned lists are appended to those lists in
  // arrival order (stable, like the reference's per-list append).  first_row = global number of row 0; keys: per row of this call,
  // nullptr -> the global row number.  Out, per kept row: its number in the chunk, its position in the store, its key.
  // All or nothing: a label that names no list, or a list that would hold more rows than begin() was told — through rows of this very
  // call too — refuses the whole call, and the fill is where it was.
  int place(const uint32_t *labels, uint64_t n, const uint64_t *keys, uint64_t first_row, std::vector<uint64_t> &src,
            std::vector<uint64_t> &dst, std::vector<uint64_t> &kv) {
    src.clear(); dst.clear(); kv.clear();
    std::vector<uint64_t> next(cursor);
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t l = labels[i];
      if (l >= nlist) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
      if (owner[l] != shard) continue;
      if (next[l] >= dense0[l + 1]) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
      next[l] += 1;
    }
    src.reserve(n / nshards + 16); dst.reserve(n / nshards + 16); kv.reserve(n / nshards + 16);
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t l = labels[i];
      if (owner[l] != shard) continue;
      const uint64_t d = cursor[l]++;
      row_ids[d] = first_row + i;
      src.push_back(i);
      dst.push_back((uint64_t)tile0[l] * IVF_TILE_ROWS + (d - dense0[l]));
      kv.push_back(keys ? keys[i] : first_row + i);
    }
    return 0;
  }

  // Every list must be complete (NO_READY, nothing changed, while one is short).  Then: the deal order of the scan's work queue, the
  // chunk length and the levels of that order, and the rows of the i largest lists.
  // head_pct: per cent of the tiles dealt in double-length chunks; tpc_override: a fixed chunk length (0 = adaptive).
  int finish(uint32_t head_pct, uint32_t tpc_override) {
    for (uint32_t l = 0; l < nlist; ++l)
      if (cursor[l] != dense0[l + 1]) return ZVEC_HIP_ERR_NO_READY;   // fewer rows than announced
    const uint64_t tiles = local_tiles;
    // largest lists are dealt first by the scan's work queue; chunk length adapts to the index size so
    // that a search has a few items per resident work-group yet long runs per top-k warm-up
    order.resize(nlist);
    for (uint32_t l = 0; l < nlist; ++l) order[l] = l;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return size[x] > size[y]; });
    const uint64_t tpc = tiles / (4ull * 256ull * 3ull);
    tiles_per_chunk = (uint32_t)std::min<uint64_t>(32, std::max<uint64_t>(4, tpc));
    if (tpc_override) tiles_per_chunk = tpc_override;
    // The queue deals lists largest first, so the lists at the END of the order are the tail of every search: one
    // work-group streams only ~7 GB/s (5.7 TB/s over ~768 resident groups), i.e. a 4-tile item lasts ~200 us, and a
    // tail of such items leaves most of the chip idle.  Guided self-scheduling in three levels of the deal order:
    // the first half of the tiles (level 0) in chunks twice as long (fewer top-k warm-ups and list write-outs per byte
    // while everybody is busy anyway), the next quarter (level 1) at the base length, the last quarter (level 2) in
    // chunks a quarter as long.  Measured (head share 0 / 25 / 50 / 75 %): 1/8 shard 0.691 / 0.700 / 0.706 / 0.67 of
    // peak, whole 10M index 0.758 / 0.767 / 0.775 / 0.770 on one box.
    tail.assign(nlist, 1);
    uint64_t acc = 0;
    for (uint32_t i = nlist; i-- > 0;) {
      const uint32_t l = order[i];
      if (acc * 4 >= tiles) break;
      tail[l] = 2;
      acc += ivf_tiles(size[l]);
    }
    acc = 0;
    for (uint32_t i = 0; i < nlist; ++i) {
      const uint32_t l = order[i];
      if (acc * 100 >= tiles * head_pct || tail[l] == 2) break;
      tail[l] = 0;
      acc += ivf_tiles(size[l]);
    }
    // rows of the i largest local lists: the bound of what i probes can scan (small-batch route); computed here, once,
    // because searches on different contexts read it concurrently
    rows_of_largest.assign((size_t)nlist + 1, 0);
    for (uint32_t i = 0; i < nlist; ++i) rows_of_largest[i + 1] = rows_of_largest[i] + size[order[i]];
    return 0;
  }

  // dense list position -> position in the blocked store; false behind the last row
  bool store_pos(uint64_t list_pos, uint64_t *pos) const {
    if (list_pos >= count_local) return false;
    const uint32_t l = (uint32_t)(std::upper_bound(dense0.begin(), dense0.end(), list_pos) - dense0.begin()) - 1;
    *pos = (uint64_t)tile0[l] * IVF_TILE_ROWS + (list_pos - dense0[l]);
    return true;
  }

  // label of every row of lists stored back to back (row i of list l: list_offsets[l] <= i < list_offsets[l + 1]; rows in front of
  // the first offset go to list 0); offsets that descend are refused before a label is written
  static int labels_of_offsets(const uint64_t *list_offsets, uint32_t nlist_, std::vector<uint32_t> &labels) {
    for (uint32_t l = 0; l < nlist_; ++l)
      if (list_offsets[l + 1] < list_offsets[l]) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    labels.assign(list_offsets[nlist_], 0);
    for (uint32_t l = 0; l < nlist_; ++l)
      for (uint64_t i = list_offsets[l]; i < list_offsets[l + 1]; ++i) labels[i] = l;
    return 0;
  }

  // rows per list of `n` labelled rows; a label that names no list is refused
  static int count_sizes(const uint32_t *labels, uint64_t n, uint32_t nlist_, std::vector<uint32_t> &sizes) {
    sizes.assign(nlist_, 0);
    for (uint64_t i = 0; i < n; ++i) {
      if (labels[i] >= nlist_) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
      sizes[labels[i]] += 1;
    }
    return 0;
  }
};
