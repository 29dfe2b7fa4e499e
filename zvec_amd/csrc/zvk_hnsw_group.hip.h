// zvk_hnsw_group.hip.h — group-by search on a built HNSW graph (zvec_hip_hnsw_search_grouped*, api_entry_hnsw_group.inc.h): the
// rule "Group-by" of DESIGN §3c, which restates HnswAlgorithm::expand_neighbors_by_group (hnsw_algorithm.cc:280-392) and
// HnswContext::topk_to_group_result (hnsw_context.h:188-250).  One wave per query, as hnsw_search_kernel: G1 is that kernel's own
// steps 1-3 (hnsw_greedy and hnsw_beam of zvk_hnsw.hip.h, untouched) with ef_eff = max(ef, group_num * group_topk); G2-G4 follow in
// the same wave on the R and C the walk left in LDS.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// A query keeps at most group_num slots.  A slot is a group number, a size and group_topk (distance, node) words ascending: the
// best documents offered to that group so far.  Without G3 the groups arrive best first and the slots beyond the group_num-th are
// never opened; with G3 fewer than group_num groups exist until the stage ends, so group_num slots always suffice.
#pragma once
#include "zvk_hnsw.hip.h"

namespace zvk {

struct HnswGroupArgs {
  const uint32_t *group_of;   // [n] group number of every node; >= ngroups: the node has no group
  uint32_t ngroups, gnum, gk; // gnum * gk <= HNSW_MAX_EF
  uint32_t *out_groups;       // [nq][gnum]
  uint32_t *out_ngroups;      // [nq]
};                            // (HnswArgs: out_keys / out_scores [nq][gnum][gk], out_counts [nq][gnum], ef = ef_eff; topk is not read)

// the search's LDS (hnsw_search_lds_bytes), then the slots
__host__ __device__ inline size_t hnsw_group_lds_bytes(size_t walk_bytes, uint32_t gnum, uint32_t gk) {
  return walk_bytes + (size_t)gnum * gk * 8 + (size_t)gnum * 8;
}

// the slots of one query, in LDS
struct HnswSlots {
  uint64_t *docs;             // [gnum][gk]
  uint32_t *group, *size;     // [gnum]
  uint32_t used;
};

// the slot that holds group g, or IDX_NONE: 64 slot numbers and one ballot per step
__device__ __forceinline__ uint32_t hnsw_slot_of(const HnswSlots &s, uint32_t g, int lane) {
  for (uint32_t j0 = 0; j0 < s.used; j0 += 64) {
    const uint32_t j = j0 + (uint32_t)lane;
    const uint64_t at = __ballot(j < s.used && s.group[j] == g);
    if (at != 0) return j0 + (uint32_t)__builtin_ctzll(at);
  }
  return IDX_NONE;
}

// Offers word w to group g: into its slot (a new one while there is room), keeping the slot's gk smallest words ascending.  A group
// met when every slot is taken is ignored: that happens in G2 alone, where it is a group past the group_num-th best.
__device__ __forceinline__ void hnsw_offer(HnswSlots &s, const HnswGroupArgs &ga, uint32_t g, uint64_t w, int lane) {
  uint32_t at = hnsw_slot_of(s, g, lane);
  if (at == IDX_NONE) {
    if (s.used == ga.gnum) return;
    at = s.used++;
    if (lane == 0) { s.group[at] = g; s.size[at] = 0; }
    hnsw_sync(false);
  }
  const uint32_t size = hnsw_put(s.docs + (size_t)at * ga.gk, hnsw_uni(s.size[at]), ga.gk, w, lane, false);
  if (lane == 0) s.size[at] = size;
  hnsw_sync(false);
}

// The candidate set of G3: C of hnsw_beam under the same rules (ascending words, a window [head, head + size) of a buffer of `buf`
// words that starts in LDS and moves, once, into the walk's workspace region G of a.ccap words; a full C loses its largest word).
struct HnswCand {
  uint64_t *C, *G;
  uint32_t head, size, buf;
  bool glob;

  __device__ __forceinline__ uint64_t pop() {
    const uint64_t top = hnsw_uni64(C[head]);
    ++head; --size;
    return top;
  }

  __device__ __forceinline__ void put(uint64_t w, uint32_t ccap, int lane) {
    if (head + size == buf) {
      if (head > 0) {                                    // slide the words down to the start of the buffer
        for (uint32_t j0 = 0; j0 < size; j0 += 64) {
          const uint32_t jj = j0 + (uint32_t)lane;
          uint64_t t = 0;
          if (jj < size) t = C[head + jj];
          hnsw_sync(glob);
          if (jj < size) C[jj] = t;
          hnsw_sync(glob);
        }
        head = 0;
      } else if (!glob && G != nullptr) {                // LDS is full of live candidates: go on in the walk's workspace region
        for (uint32_t jj = (uint32_t)lane; jj < size; jj += 64) G[jj] = C[jj];
        C = G;
        buf = ccap;
        glob = true;
        hnsw_sync(true);
      }
    }
    size = hnsw_put(C + head, size, buf - head, w, lane, glob);
  }
};

// G3 of the rule: walks on from the members of R until gnum groups have been offered a document, C is empty or the scan limit is
// reached.  C: the HNSW_C_LDS words in LDS, G: the walk's workspace region (null when a.ccap fits LDS), vis: the walk's visited bits.
template <typename S>
__device__ __forceinline__ void hnsw_group_expand(const HnswArgs &a, const HnswGroupArgs &ga, S score, HnswSlots &s, const uint64_t *R,
                                                  uint32_t rsize, uint64_t *C, uint64_t *G, uint32_t *coll, float *cdist, uint32_t *vis,
                                                  uint32_t &scanned, uint32_t &hops, int lane) {
  // (a walk that may go on has computed fewer than max_scan distances, and every member of R is a distinct node among them: R fits C)
  if (!(scanned < a.max_scan)) return;
  for (uint32_t i = (uint32_t)lane; i < a.vis_words; i += 64) vis[i] = 0;
  hnsw_sync(true);
  for (uint32_t i = (uint32_t)lane; i < rsize; i += 64) {
    const uint64_t w = R[i];
    const uint32_t id = (uint32_t)w;
    atomicOr(&vis[id >> 5], 1u << (id & 31u));
    C[i] = w;
  }
  hnsw_sync(true);
  HnswCand c{C, G, 0, rsize, min(HNSW_C_LDS, a.ccap), false};
  while (c.size > 0 && scanned < a.max_scan) {
    const uint64_t top = c.pop();
    ++hops;
    uint32_t cnt;
    const uint32_t *lst = hnsw_list(a, 0, (uint32_t)top, cnt);
    for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
      const uint32_t nl = min(64u, cnt - c0);
      const bool valid = (uint32_t)lane < nl;
      const uint32_t id = valid ? lst[c0 + lane] : 0u;
      bool dup = false;                                  // the same id earlier in this list: only its first place counts
      for (uint32_t b = 0; b + 1 < nl; ++b) dup = dup || ((uint32_t)lane > b && id == bcast_u(id, (int)b));
      bool fresh = false;
      if (valid && !dup) fresh = ((atomicOr(&vis[id >> 5], 1u << (id & 31u)) >> (id & 31u)) & 1u) == 0;
      const uint64_t fm = __ballot(fresh);
      const uint32_t nc = (uint32_t)__popcll(fm);
      if (nc == 0) continue;
      if (fresh) coll[__popcll(fm & ((1ull << lane) - 1ull))] = id;
      hnsw_sync(false);
      score(a, coll, cdist, nc, lane);                   // the whole pass at once; applied in list order below
      // lane j holds collected node j: its word and the group it may be offered to
      uint64_t wj = 0;
      uint32_t gj = IDX_NONE;
      if ((uint32_t)lane < nc) {
        const uint32_t v = coll[lane];
        wj = hnsw_pack(cdist[lane], v);
        if (!hnsw_excluded(a, v)) gj = ga.group_of[v];
      }
      for (uint32_t j = 0; j < nc; ++j) {
        ++scanned;
        const uint32_t g = bcast_u(gj, (int)j);
        const uint64_t w = bcast_u64(wj, (int)j);
        if (g < ga.ngroups) {
          hnsw_offer(s, ga, g, w, lane);
          if (s.used == ga.gnum) return;                 // the stage ends with this node: it is counted and not inserted
        }
        c.put(w, a.ccap, lane);
      }
      hnsw_sync(false);
    }
  }
}

// G4 for query q of the launch: the slots best first (by first word), their documents, the counts within the threshold; unused
// places as zvec_hip_flat_search_grouped leaves them.  `order` is gnum words of LDS that nothing else uses any more.
__device__ __forceinline__ void hnsw_group_emit(const HnswArgs &a, const HnswGroupArgs &ga, uint32_t q, const HnswSlots &s, uint32_t *order,
                                                uint32_t scanned, uint32_t hops, int lane) {
  const uint32_t gnum = ga.gnum, gk = ga.gk;
  for (uint32_t t = (uint32_t)lane; t < s.used; t += 64) {       // the words are distinct: the rank is the number of smaller first words
    const uint64_t mine = s.docs[(size_t)t * gk];
    uint32_t rank = 0;
    for (uint32_t u = 0; u < s.used; ++u) rank += s.docs[(size_t)u * gk] < mine ? 1u : 0u;
    order[rank] = t;
  }
  hnsw_sync(false);
  for (uint32_t r = (uint32_t)lane; r < gnum; r += 64) {
    uint32_t group = IDX_NONE, keep = 0;
    if (r < s.used) {
      const uint32_t t = order[r];
      group = s.group[t];
      for (uint32_t j = 0; j < s.size[t]; ++j) keep += fkey_inv((uint32_t)(s.docs[(size_t)t * gk + j] >> 32)) <= a.threshold ? 1u : 0u;
    }
    a.out_counts[(size_t)q * gnum + r] = keep;
    ga.out_groups[(size_t)q * gnum + r] = group;
  }
  const uint32_t places = gnum * gk;
  for (uint32_t i = (uint32_t)lane; i < places; i += 64) {       // consecutive lanes, consecutive places of the output
    const uint32_t r = i / gk, j = i - r * gk;
    uint64_t key = ~0ull;
    float d = __builtin_inff();
    if (r < s.used) {
      const uint32_t t = order[r];
      if (j < s.size[t]) {
        const uint64_t w = s.docs[(size_t)t * gk + j];
        key = a.keys[(uint32_t)w];
        d = fkey_inv((uint32_t)(w >> 32));
      }
    }
    a.out_keys[(size_t)q * places + i] = key;
    a.out_scores[(size_t)q * places + i] = d;
  }
  if (lane == 0) {
    ga.out_ngroups[q] = s.used;
    a.stats[2 * (size_t)q] = scanned;
    a.stats[2 * (size_t)q + 1] = hops;
  }
}

template <HnswKind K>
__global__ __launch_bounds__(64) void hnsw_group_search_kernel(HnswArgs a, HnswGroupArgs ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_smem[];
  typedef typename HnswDenseKind<K>::lds lds_t;
  const int lane = (int)threadIdx.x;
  const uint32_t q = blockIdx.x;
  lds_t *qv = reinterpret_cast<lds_t *>(hnsw_smem);
  uint64_t *R = reinterpret_cast<uint64_t *>(qv + a.dpad);
  uint64_t *C = R + a.ef;
  uint32_t *coll = reinterpret_cast<uint32_t *>(C + HNSW_C_LDS);
  float *cdist = reinterpret_cast<float *>(coll + 64);
  HnswSlots s;
  s.docs = reinterpret_cast<uint64_t *>(cdist + 64);
  s.group = reinterpret_cast<uint32_t *>(s.docs + (size_t)ga.gnum * ga.gk);
  s.size = s.group + ga.gnum;
  s.used = 0;
  for (uint32_t i = (uint32_t)lane; i < a.dpad; i += 64) qv[i] = i < a.dim ? HnswDenseKind<K>::word(a.queries, (size_t)q * a.dim + i) : lds_t(0);
  if (lane == 0) coll[0] = a.entry;
  hnsw_sync(false);
  const typename HnswRows<K>::Scorer score{qv};

  // G1: steps 1-3 of the plain rule under ef_eff
  uint32_t scanned = 1, hops = 0, ep = a.entry;
  score(a, coll, cdist, 1, lane);
  float dist = cdist[0];
  hnsw_sync(false);
  for (uint32_t l = a.max_level; l >= 1; --l) hnsw_greedy(a, l, score, coll, cdist, ep, dist, scanned, lane);
  uint64_t *G = a.cand_ws != nullptr ? a.cand_ws + (size_t)q * a.ccap : nullptr;
  uint32_t *vis = a.visited + (size_t)q * a.vis_words;
  const uint32_t rsize = hnsw_beam(a, 0, score, R, C, G, coll, cdist, vis, ep, dist, scanned, hops, lane);

  // G2: R ascending, each member offered to its group; 64 group numbers are fetched at a time
  for (uint32_t i0 = 0; i0 < rsize; i0 += 64) {
    const uint32_t i = i0 + (uint32_t)lane;
    uint64_t wi = 0;
    uint32_t gi = IDX_NONE;
    if (i < rsize) { wi = R[i]; gi = ga.group_of[(uint32_t)wi]; }
    const uint32_t nl = min(64u, rsize - i0);
    for (uint32_t j = 0; j < nl; ++j) {
      const uint32_t g = bcast_u(gi, (int)j);
      if (g < ga.ngroups) hnsw_offer(s, ga, g, bcast_u64(wi, (int)j), lane);
    }
  }

  // G3: fewer groups than asked for: walk on
  if (s.used < ga.gnum) hnsw_group_expand(a, ga, score, s, R, rsize, C, G, coll, cdist, vis, scanned, hops, lane);

  // G4 (C's place in LDS is free now: it holds the order of the slots)
  hnsw_sync(false);
  hnsw_group_emit(a, ga, q, s, reinterpret_cast<uint32_t *>(C), scanned, hops, lane);
}

// an index without rows: no groups (keys, scores and statistics are hnsw_empty_kernel's)
__global__ void hnsw_group_empty_kernel(HnswGroupArgs ga, uint32_t *out_counts, uint32_t nq) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (uint64_t)nq * ga.gnum) {
    ga.out_groups[i] = IDX_NONE;
    out_counts[i] = 0;
  }
  if (i < nq) ga.out_ngroups[i] = 0;
}

}  // namespace zvk
