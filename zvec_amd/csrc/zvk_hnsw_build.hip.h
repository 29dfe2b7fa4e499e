// zvk_hnsw_build.hip.h — building an HNSW graph in rounds (zvec_hip_hnsw_build, api_entry_hnsw_build.inc.h) by the rule of DESIGN §3c
// "Building", which restates HnswAlgorithm::add_node, update_neighbors and reverse_update_neighbors (hnsw_algorithm.cc:31-81, 394-515)
// for a round of nodes that all search the graph as it stood when the round began.
//   hnsw_insert_kernel   one wave per new node: descent, one beam search per level, selection; writes the node's own lists (nobody
//                        reads them during the round) and one request word per selected neighbour into the round buffer
//   (device radix sort of the request words: level, target, source)
//   hnsw_groups_kernel   the first word of every (level, target) group
//   hnsw_reverse_kernel  one wave per group applies its requests in ascending source
//   hnsw_reverse_one_kernel  a round of ONE node: every used request word is a group of one, no sort and no grouping
//   hnsw_restride_kernel the upper table under a larger stride (zvec_hip_hnsw_add, api_entry_hnsw_add.inc.h)
// The walk is the search's own (hnsw_greedy, hnsw_beam, hnsw_put, hnsw_distances of zvk_hnsw.hip.h), and so is the template parameter
// H (rows are halves): a row copied into LDS is widened on the way and kept there as fp32.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
#pragma once
#include <hipcub/hipcub.hpp>
#include "zvk_hnsw.hip.h"

namespace zvk {

constexpr uint32_t HNSW_BUILD_MAX_LEVEL = 15;
constexpr uint32_t HNSW_BUILD_MAX_M0 = 256;      // the kept ids of one selection are held in LDS
constexpr uint32_t HNSW_BUILD_MAX_M = 128;
constexpr uint32_t HNSW_REQ_SRC_BITS = 28;       // a request word: level << 60 | target << 28 | source - first node of the round
constexpr uint64_t HNSW_REQ_NONE = ~0ull;        // (no target is 2^32 - 1: sorts behind every request, belongs to no group)

struct HnswBuildArgs {
  HnswArgs g;                   // the frozen graph: ef = ef_construction, max_scan = 2^32 - 1, no exclude bits, entry = the round's
                                // entry point, ccap = nodes in the graph; visited / cand_ws are the slice's regions, one per wave
  uint32_t *nbr0, *cnt0, *nbr_up, *cnt_up;       // the same lists, writable
  uint32_t node_base;           // levels and req_off cover the nodes from this one on: 0 in a build, the old node count in an append
  const uint32_t *levels;       // [nodes from node_base]
  const uint64_t *req_off;      // [nodes from node_base + 1] first request slot of every such node, counted from node node_base
  uint64_t req_base;            // req_off[first node of the round]
  uint64_t *req;                // the round buffer
  uint32_t round_first, first, top;              // first: the first node of this slice
  uint32_t prune_cnt, min_neighbors;
  unsigned long long *counters; // distances computed by the insert kernels, requests raised, prunes run
};

__host__ __device__ inline size_t hnsw_insert_lds_bytes(uint32_t dpad, uint32_t ef) {
  return (size_t)dpad * 8 + (size_t)ef * 8 + (size_t)HNSW_C_LDS * 8 + 64 * 4 + 64 * 4 + HNSW_BUILD_MAX_M0 * 4 + 16 * 4;
}
__host__ __device__ inline size_t hnsw_reverse_lds_bytes(uint32_t dpad) {
  return (size_t)dpad * 8 + (size_t)(HNSW_BUILD_MAX_M0 + 1) * 8 + 8 + 64 * 4 + 64 * 4 + HNSW_BUILD_MAX_M0 * 4;
}

// The keep rule of update_neighbors / reverse_update_neighbors: walk the ns words of S (ascending by (distance to the base, id)) and keep
// c unless some kept s has d(c, s) <= d(c, base); stop at cap.  The candidate's row goes into cv, its distances to the kept ids are
// computed 64 at a time and one ballot decides.  kept[] receives the ids, mask (nullable) the bit of every kept place of S; ndist
// grows by the kept ids each candidate was compared with.  Returns the number kept.
template <bool H>
__device__ __forceinline__ uint32_t hnsw_keep(const HnswArgs &a, const uint64_t *S, uint32_t ns, uint32_t cap, float *cv, uint32_t *kept,
                                              uint32_t *mask, float *cdist, uint32_t &ndist, int lane) {
  uint32_t nk = 0;
  for (uint32_t j = 0; j < ns && nk < cap; ++j) {
    const uint64_t w = hnsw_uni64(S[j]);
    const uint32_t c = (uint32_t)w;
    const float dc = fkey_inv((uint32_t)(w >> 32));
    bool bad = false;
    if (nk > 0) {
      for (uint32_t t = (uint32_t)lane; t < a.dpad; t += 64) cv[t] = hnsw_elem<H>(a.rows, (size_t)c * a.dpad + t);
      hnsw_sync(false);
      for (uint32_t k0 = 0; k0 < nk; k0 += 64) {
        const uint32_t nc = min(64u, nk - k0);
        hnsw_distances<H>(a, cv, kept + k0, cdist, nc, lane);
        bad = bad || __ballot((uint32_t)lane < nc && cdist[lane] <= dc) != 0;
        hnsw_sync(false);
      }
      ndist += nk;
    }
    if (!bad) {
      if (lane == 0) {
        kept[nk] = c;
        if (mask != nullptr) mask[j >> 5] |= 1u << (j & 31u);
      }
      ++nk;
      hnsw_sync(false);
    }
  }
  return nk;
}

template <bool H>
__global__ __launch_bounds__(64) void hnsw_insert_kernel(HnswBuildArgs b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_smem[];
  const HnswArgs &a = b.g;
  const int lane = (int)threadIdx.x;
  const uint32_t wv = blockIdx.x, i = b.first + wv;
  float *qv = reinterpret_cast<float *>(hnsw_smem);
  float *cv = qv + a.dpad;
  uint64_t *R = reinterpret_cast<uint64_t *>(cv + a.dpad);
  uint64_t *C = R + a.ef;
  uint32_t *coll = reinterpret_cast<uint32_t *>(C + HNSW_C_LDS);
  float *cdist = reinterpret_cast<float *>(coll + 64);
  uint32_t *kept = reinterpret_cast<uint32_t *>(cdist + 64);
  uint32_t *mask = kept + HNSW_BUILD_MAX_M0;
  const uint32_t li = hnsw_uni(b.levels[i - b.node_base]);
  for (uint32_t t = (uint32_t)lane; t < a.dpad; t += 64) qv[t] = hnsw_elem<H>(a.rows, (size_t)i * a.dpad + t);
  if (lane == 0) coll[0] = a.entry;
  hnsw_sync(false);

  // 1. the entry point, then greedy on the levels above the node's own
  uint32_t scanned = 1, hops = 0, ep = a.entry;
  hnsw_distances<H>(a, qv, coll, cdist, 1, lane);
  float dist = cdist[0];
  hnsw_sync(false);
  for (uint32_t l = b.top; l > li; --l) hnsw_greedy<H>(a, l, qv, coll, cdist, ep, dist, scanned, lane);

  uint32_t *vis = a.visited + (size_t)wv * a.vis_words;
  uint64_t *G = a.cand_ws != nullptr ? a.cand_ws + (size_t)wv * a.ccap : nullptr;
  uint64_t *req = b.req + (hnsw_uni64(b.req_off[i - b.node_base]) - b.req_base);
  uint32_t nreq = 0;
  for (int l = (int)min(li, b.top); l >= 0; --l) {
    const uint32_t cap = l == 0 ? a.m0 : a.m;
    // 2. W = the beam search's result list on this level; its nearest is the next level's entry point
    for (uint32_t t = (uint32_t)lane; t < a.vis_words; t += 64) vis[t] = 0;
    hnsw_sync(true);
    const uint32_t rsize = hnsw_beam<H>(a, (uint32_t)l, qv, R, C, G, coll, cdist, vis, ep, dist, scanned, hops, lane);
    {
      const uint64_t w0 = hnsw_uni64(R[0]);
      ep = (uint32_t)w0;
      dist = fkey_inv((uint32_t)(w0 >> 32));
    }
    // 3. selection
    uint32_t nk;
    if (rsize <= min(b.prune_cnt, cap)) {
      for (uint32_t j = (uint32_t)lane; j < rsize; j += 64) kept[j] = (uint32_t)R[j];
      nk = rsize;
      hnsw_sync(false);
    } else {
      if (lane < 16) mask[lane] = 0;
      hnsw_sync(false);
      nk = hnsw_keep<H>(a, R, rsize, cap, cv, kept, mask, cdist, scanned, lane);
      for (uint32_t j = 0; j < rsize && nk < b.min_neighbors; ++j) {
        if ((hnsw_uni(mask[j >> 5]) >> (j & 31u)) & 1u) continue;
        if (lane == 0) kept[nk] = (uint32_t)R[j];
        ++nk;
      }
      hnsw_sync(false);
    }
    // 4. the node's own list, and one request per selected neighbour
    uint32_t *own, *ocnt;
    if (l == 0) {
      own = b.nbr0 + (size_t)i * a.m0;
      ocnt = b.cnt0 + i;
    } else {
      const size_t slot = (size_t)hnsw_uni(a.upper_of[i]) * a.max_level + (uint32_t)(l - 1);
      own = b.nbr_up + slot * a.m;
      ocnt = b.cnt_up + slot;
    }
    for (uint32_t j = (uint32_t)lane; j < cap; j += 64) {
      uint64_t word = HNSW_REQ_NONE;
      if (j < nk) {
        const uint32_t t = kept[j];
        own[j] = t;
        word = ((uint64_t)(uint32_t)l << 60) | ((uint64_t)t << HNSW_REQ_SRC_BITS) | (uint64_t)(i - b.round_first);
      }
      req[j] = word;
    }
    if (lane == 0) *ocnt = nk;
    req += cap;
    nreq += nk;
    hnsw_sync(false);
  }
  if (lane == 0) {
    atomicAdd(&b.counters[0], (unsigned long long)scanned);
    atomicAdd(&b.counters[1], (unsigned long long)nreq);
  }
}

// gstart[0 .. *ngroups): the index of the first word of every (level, target) group of the sorted round buffer, in no order
__global__ void hnsw_groups_kernel(const uint64_t *req, uint64_t slots, uint32_t *gstart, uint32_t *ngroups) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= slots) return;
  const uint64_t w = req[j];
  if (w == HNSW_REQ_NONE) return;
  if (j == 0 || (req[j - 1] >> HNSW_REQ_SRC_BITS) != (w >> HNSW_REQ_SRC_BITS)) gstart[atomicAdd(ngroups, 1u)] = (uint32_t)j;
}

// The LDS of a reverse wave (hnsw_reverse_lds_bytes)
struct HnswReverseLds {
  float *qv, *cv, *cdist;
  uint64_t *S;
  uint32_t *coll, *kept;
  __device__ explicit HnswReverseLds(unsigned char *smem, uint32_t dpad) {
    qv = reinterpret_cast<float *>(smem);
    cv = qv + dpad;
    S = reinterpret_cast<uint64_t *>(cv + dpad);
    coll = reinterpret_cast<uint32_t *>(S + HNSW_BUILD_MAX_M0 + 2);
    cdist = reinterpret_cast<float *>(coll + 64);
    kept = reinterpret_cast<uint32_t *>(cdist + 64);
  }
};

// One (level, target) group, by one wave: the words req[j0 .. ) that share req[j0]'s level and target, at most up to jend, in
// ascending source.  A list with room takes the source at its end; a full list plus the source is sorted by (distance to the target,
// id) and goes through the keep rule, no shortcut and no fill, and the places the prune emptied are zeroed, so that a list never keeps
// anything behind its count.  Returns the prunes run.
template <bool H>
__device__ __forceinline__ uint32_t hnsw_reverse_group(const HnswBuildArgs &b, const HnswReverseLds &m, const uint64_t *req, uint64_t j0,
                                                       uint64_t jend, int lane) {
  const HnswArgs &a = b.g;
  const uint64_t head = hnsw_uni64(req[j0]) >> HNSW_REQ_SRC_BITS;
  const uint32_t l = (uint32_t)(head >> 32), t = (uint32_t)head;
  const uint32_t cap = l == 0 ? a.m0 : a.m;
  uint32_t *lst, *lcnt;
  if (l == 0) {
    lst = b.nbr0 + (size_t)t * a.m0;
    lcnt = b.cnt0 + t;
  } else {
    const size_t slot = (size_t)hnsw_uni(a.upper_of[t]) * a.max_level + (l - 1);
    lst = b.nbr_up + slot * a.m;
    lcnt = b.cnt_up + slot;
  }
  uint32_t cnt = hnsw_uni(*lcnt), nprune = 0;
  bool have_row = false;
  for (uint64_t j = j0; j < jend; ++j) {
    const uint64_t w = hnsw_uni64(req[j]);
    if ((w >> HNSW_REQ_SRC_BITS) != head) break;
    const uint32_t src = b.round_first + (uint32_t)(w & ((1ull << HNSW_REQ_SRC_BITS) - 1ull));
    if (cnt < cap) {
      if (lane == 0) lst[cnt] = src;
      ++cnt;
      hnsw_sync(true);
      continue;
    }
    if (!have_row) {
      for (uint32_t x = (uint32_t)lane; x < a.dpad; x += 64) m.qv[x] = hnsw_elem<H>(a.rows, (size_t)t * a.dpad + x);
      have_row = true;
      hnsw_sync(false);
    }
    uint32_t ssize = 0;
    for (uint32_t c0 = 0; c0 < cap + 1; c0 += 64) {
      const uint32_t nc = min(64u, cap + 1 - c0);
      if ((uint32_t)lane < nc) m.coll[lane] = c0 + (uint32_t)lane < cap ? lst[c0 + lane] : src;
      hnsw_sync(false);
      hnsw_distances<H>(a, m.qv, m.coll, m.cdist, nc, lane);
      for (uint32_t jj = 0; jj < nc; ++jj) {
        const uint64_t word = hnsw_pack(__builtin_bit_cast(float, hnsw_uni(__builtin_bit_cast(uint32_t, m.cdist[jj]))), hnsw_uni(m.coll[jj]));
        ssize = hnsw_put(m.S, ssize, cap + 1, word, lane, false);
      }
      hnsw_sync(false);
    }
    uint32_t unused = 0;
    const uint32_t nk = hnsw_keep<H>(a, m.S, ssize, cap, m.cv, m.kept, nullptr, m.cdist, unused, lane);
    for (uint32_t x = (uint32_t)lane; x < cap; x += 64) lst[x] = x < nk ? m.kept[x] : 0u;
    cnt = nk;
    ++nprune;
    hnsw_sync(true);
  }
  if (lane == 0) *lcnt = cnt;
  return nprune;
}

// One wave per (level, target) group of the sorted round buffer, grid-stride.  Targets are older than the round and every
// (level, target) is one group, so no two waves touch one list.
template <bool H>
__global__ __launch_bounds__(64) void hnsw_reverse_kernel(HnswBuildArgs b, const uint64_t *req, uint64_t slots, const uint32_t *gstart,
                                                          const uint32_t *ngroups) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_smem[];
  const int lane = (int)threadIdx.x;
  const HnswReverseLds m(hnsw_smem, b.g.dpad);
  const uint32_t ng = hnsw_uni(*ngroups);
  uint32_t nprune = 0;
  for (uint32_t g = blockIdx.x; g < ng; g += gridDim.x) nprune += hnsw_reverse_group<H>(b, m, req, hnsw_uni(gstart[g]), slots, lane);
  if (lane == 0 && nprune != 0) atomicAdd(&b.counters[2], (unsigned long long)nprune);
}

// The reverse phase of a round of ONE node, on the round buffer as the insert kernel left it: one wave per request slot, grid-stride.
// The selection of one node on one level holds distinct targets, so the used words are distinct (level, target) pairs with one source
// each: every used word is a whole group, and no two waves touch one list.
template <bool H>
__global__ __launch_bounds__(64) void hnsw_reverse_one_kernel(HnswBuildArgs b, uint64_t slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_smem[];
  const int lane = (int)threadIdx.x;
  const HnswReverseLds m(hnsw_smem, b.g.dpad);
  uint32_t nprune = 0;
  for (uint64_t j = blockIdx.x; j < slots; j += gridDim.x) {
    if (hnsw_uni64(b.req[j]) == HNSW_REQ_NONE) continue;
    nprune += hnsw_reverse_group<H>(b, m, b.req, j, j + 1, lane);
  }
  if (lane == 0 && nprune != 0) atomicAdd(&b.counters[2], (unsigned long long)nprune);
}

// The upper table under a larger stride: old slot (u, l) goes to new slot (u, l); the new arrays are zero on entry.  One thread per
// old neighbour place, and per old count.
__global__ void hnsw_restride_kernel(const uint32_t *old_nbr, const uint32_t *old_cnt, uint32_t *new_nbr, uint32_t *new_cnt, uint64_t n_upper,
                                     uint32_t old_stride, uint32_t new_stride, uint32_t m) {
  const uint64_t per = (uint64_t)old_stride * m;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_upper * per) {
    const uint64_t u = i / per, r = i % per;           // r = l * m + place
    new_nbr[u * new_stride * m + r] = old_nbr[i];
  }
  if (i < n_upper * old_stride) new_cnt[(i / old_stride) * new_stride + i % old_stride] = old_cnt[i];
}

}  // namespace zvk
