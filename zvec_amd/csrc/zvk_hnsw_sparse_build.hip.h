// zvk_hnsw_sparse_build.hip.h — building an HNSW graph over SPARSE rows in rounds (zvec_hip_hnsw_sparse_build,
// api_entry_hnsw_sparse_build.inc.h) by the rule of DESIGN §3c "Building", unchanged: the round structure, the request words, their
// sort and hnsw_groups_kernel are zvk_hnsw_build.hip.h's, the walk is zvk_hnsw.hip.h's (hnsw_greedy, hnsw_beam, hnsw_put), and the
// distance is zvk_hnsw_sparse.hip.h's HnswSparseScorer.  Reference: hnsw_sparse_algorithm.cc (add_node, update_neighbors,
// reverse_update_neighbors), which is hnsw_algorithm.cc line for line but for dc.dist(..) on a sparse row.
//   hnsw_sparse_insert_kernel       one wave per new node: descent, one beam search per level, selection, own lists, request words
//   hnsw_sparse_reverse_kernel      one wave per (level, target) group of the sorted round buffer
//   hnsw_sparse_reverse_one_kernel  a round of ONE node: every used request word is a group of one
// A sparse score is index matching, not a dense product: there is nothing here for the matrix cores, and no inline assembly.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Two runs in LDS.  The scorer wants one operand staged in LDS (indices, then values as stored) and streams the other from CSR,
// sixteen lanes a row, four rows in flight per wave.  Run A is the BASE of the wave's work: the new node's row in the insert kernel,
// the target's row in a reverse group (staged only when the group's first prune is due).  Run B is the keep rule's current candidate
// c, staged once per candidate; the kept ids are scored against it 64 at a time and one ballot decides.  Both runs are sized by the
// longest row of the call, which the host knows from the counts.
//
// Roles.  A score's bits depend on the (staged run, streamed row) pair alone, as in the search.  d(c, s) of the keep rule is
// (c staged, s streamed); it is compared with d(c, base), which came out of the walk or the sort as (base staged, c streamed).  On
// real values the two roles may differ in the last bit; integer-valued data is exact either way.  An empty staged run reads nothing
// and scores +0.
//
// LDS (hnsw_sparse_build_lds_bytes): run A | run B | R [words] | C [HNSW_C_LDS] | row begins [64] (u64) | coll [64] | cdist [64] |
// row lengths [64] | kept [256] | mask [16].  The insert kernel's R has ef_construction words; the reverse kernels keep their sorted
// list of at most m0 + 1 words there (HNSW_BUILD_MAX_M0 + 2 words) and have no C.
#pragma once
#include "zvk_hnsw_build.hip.h"
#include "zvk_hnsw_sparse.hip.h"

namespace zvk {

struct HnswSparseBuildArgs {
  HnswBuildArgs b;            // as the dense build's; of b.g rows, dim, dpad, ip and queries are not read
  const uint64_t *row_off;    // [nodes + 1] the rows, CSR
  const uint32_t *idx;
  const void *val;            // of the kernel's VT
  uint32_t run_elems;         // the longest row of the call: what each of the two runs has room for
};

__host__ __device__ inline size_t hnsw_sparse_build_lds_bytes(uint32_t run_elems, uint32_t width, uint32_t words, bool cand) {
  return 2 * hnsw_sparse_run_bytes(run_elems, width) + (size_t)words * 8 + (cand ? (size_t)HNSW_C_LDS * 8 : 0) + 64 * 8 + 3 * 64 * 4 +
         HNSW_BUILD_MAX_M0 * 4 + 16 * 4;
}

struct HnswSparseBuildLds {
  unsigned char *run_a, *run_b;
  uint64_t *R, *C, *rbeg;
  uint32_t *coll, *rlen, *kept, *mask;
  float *cdist;
  __device__ HnswSparseBuildLds(unsigned char *smem, size_t run_bytes, uint32_t words, bool cand) {
    run_a = smem;
    run_b = run_a + run_bytes;
    R = reinterpret_cast<uint64_t *>(run_b + run_bytes);
    C = R + words;
    rbeg = C + (cand ? HNSW_C_LDS : 0u);
    coll = reinterpret_cast<uint32_t *>(rbeg + 64);
    cdist = reinterpret_cast<float *>(coll + 64);
    rlen = reinterpret_cast<uint32_t *>(cdist + 64);
    kept = rlen + 64;
    mask = kept + HNSW_BUILD_MAX_M0;
  }
};

// The whole wave copies the stored row of `node` into the run at `run` (indices, then values as stored) and returns the scorer of
// the other rows against it.  Whoever staged the run's last occupant has finished reading it (every scorer call ends in hnsw_sync).
template <typename VT>
__device__ __forceinline__ HnswSparseScorer<VT> hnsw_sparse_stage_row(const HnswSparseBuildArgs &s, const HnswSparseBuildLds &m,
                                                                      unsigned char *run, uint32_t node, int lane) {
  const VT *val = static_cast<const VT *>(s.val);
  const uint64_t rb = hnsw_uni64(s.row_off[node]);
  const uint32_t len = (uint32_t)min((uint64_t)s.run_elems, hnsw_uni64(s.row_off[(size_t)node + 1]) - rb);
  uint32_t *qi = reinterpret_cast<uint32_t *>(run);
  VT *qv = reinterpret_cast<VT *>(qi + len);
  for (uint32_t e = (uint32_t)lane; e < len; e += 64) {
    qi[e] = s.idx[rb + e];
    qv[e] = val[rb + e];
  }
  hnsw_sync(false);
  return HnswSparseScorer<VT>{s.row_off, s.idx, val, qi, qv, len, sparse_halvings(len), m.rbeg, m.rlen};
}

// hnsw_keep on sparse rows: walk the ns words of S (ascending by (distance to the base, id)) and keep c unless some kept s has
// d(c, s) <= d(c, base); stop at cap.  c goes into run B.  m.kept receives the ids, mask (nullable) the bit of every kept place of S;
// ndist grows by the kept ids each candidate was compared with.  Returns the number kept.
template <typename VT>
__device__ __forceinline__ uint32_t hnsw_sparse_keep(const HnswSparseBuildArgs &s, const HnswSparseBuildLds &m, const uint64_t *S,
                                                     uint32_t ns, uint32_t cap, uint32_t *mask, uint32_t &ndist, int lane) {
  uint32_t nk = 0;
  for (uint32_t j = 0; j < ns && nk < cap; ++j) {
    const uint64_t w = hnsw_uni64(S[j]);
    const uint32_t c = (uint32_t)w;
    const float dc = fkey_inv((uint32_t)(w >> 32));
    bool bad = false;
    if (nk > 0) {
      const HnswSparseScorer<VT> to_c = hnsw_sparse_stage_row<VT>(s, m, m.run_b, c, lane);
      for (uint32_t k0 = 0; k0 < nk; k0 += 64) {
        const uint32_t nc = min(64u, nk - k0);
        to_c(s.b.g, m.kept + k0, m.cdist, nc, lane);
        bad = bad || __ballot((uint32_t)lane < nc && m.cdist[lane] <= dc) != 0;
        hnsw_sync(false);
      }
      ndist += nk;
    }
    if (!bad) {
      if (lane == 0) {
        m.kept[nk] = c;
        if (mask != nullptr) mask[j >> 5] |= 1u << (j & 31u);
      }
      ++nk;
      hnsw_sync(false);
    }
  }
  return nk;
}

// the writable list of node t on level l and its count
__device__ __forceinline__ uint32_t *hnsw_sparse_own_list(const HnswBuildArgs &b, uint32_t l, uint32_t t, uint32_t *&cnt) {
  if (l == 0) {
    cnt = b.cnt0 + t;
    return b.nbr0 + (size_t)t * b.g.m0;
  }
  const size_t slot = (size_t)hnsw_uni(b.g.upper_of[t]) * b.g.max_level + (l - 1);
  cnt = b.cnt_up + slot;
  return b.nbr_up + slot * b.g.m;
}

template <typename VT>
__global__ __launch_bounds__(64) void hnsw_sparse_insert_kernel(HnswSparseBuildArgs s) {
  extern __shared__ f32x4 zvk_smem4[];
  const HnswBuildArgs &b = s.b;
  const HnswArgs &a = b.g;
  const int lane = (int)threadIdx.x;
  const uint32_t wv = blockIdx.x, i = b.first + wv;
  const HnswSparseBuildLds m(reinterpret_cast<unsigned char *>(zvk_smem4), hnsw_sparse_run_bytes(s.run_elems, sizeof(VT)), a.ef, true);
  const uint32_t li = hnsw_uni(b.levels[i - b.node_base]);
  if (lane == 0) m.coll[0] = a.entry;
  const HnswSparseScorer<VT> score = hnsw_sparse_stage_row<VT>(s, m, m.run_a, i, lane);

  // 1. the entry point, then greedy on the levels above the node's own
  uint32_t scanned = 1, hops = 0, ep = a.entry;
  score(a, m.coll, m.cdist, 1, lane);
  float dist = m.cdist[0];
  hnsw_sync(false);
  for (uint32_t l = b.top; l > li; --l) hnsw_greedy(a, l, score, m.coll, m.cdist, ep, dist, scanned, lane);

  uint32_t *vis = a.visited + (size_t)wv * a.vis_words;
  uint64_t *G = a.cand_ws != nullptr ? a.cand_ws + (size_t)wv * a.ccap : nullptr;
  uint64_t *req = b.req + (hnsw_uni64(b.req_off[i - b.node_base]) - b.req_base);
  uint32_t nreq = 0;
  for (int l = (int)min(li, b.top); l >= 0; --l) {
    const uint32_t cap = l == 0 ? a.m0 : a.m;
    // 2. W = the beam search's result list on this level; its nearest is the next level's entry point
    for (uint32_t t = (uint32_t)lane; t < a.vis_words; t += 64) vis[t] = 0;
    hnsw_sync(true);
    const uint32_t rsize = hnsw_beam(a, (uint32_t)l, score, m.R, m.C, G, m.coll, m.cdist, vis, ep, dist, scanned, hops, lane);
    {
      const uint64_t w0 = hnsw_uni64(m.R[0]);
      ep = (uint32_t)w0;
      dist = fkey_inv((uint32_t)(w0 >> 32));
    }
    // 3. selection
    uint32_t nk;
    if (rsize <= min(b.prune_cnt, cap)) {
      for (uint32_t j = (uint32_t)lane; j < rsize; j += 64) m.kept[j] = (uint32_t)m.R[j];
      nk = rsize;
      hnsw_sync(false);
    } else {
      if (lane < 16) m.mask[lane] = 0;
      hnsw_sync(false);
      nk = hnsw_sparse_keep<VT>(s, m, m.R, rsize, cap, m.mask, scanned, lane);
      for (uint32_t j = 0; j < rsize && nk < b.min_neighbors; ++j) {
        if ((hnsw_uni(m.mask[j >> 5]) >> (j & 31u)) & 1u) continue;
        if (lane == 0) m.kept[nk] = (uint32_t)m.R[j];
        ++nk;
      }
      hnsw_sync(false);
    }
    // 4. the node's own list, and one request per selected neighbour
    uint32_t *ocnt;
    uint32_t *own = hnsw_sparse_own_list(b, (uint32_t)l, i, ocnt);
    for (uint32_t j = (uint32_t)lane; j < cap; j += 64) {
      uint64_t word = HNSW_REQ_NONE;
      if (j < nk) {
        const uint32_t t = m.kept[j];
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

// One (level, target) group, by one wave, as hnsw_reverse_group: the words req[j0 .. ) that share req[j0]'s level and target, at most
// up to jend, in ascending source.  A list with room takes the source at its end.  A full list plus the source is scored against
// the target's row (run A, staged at the group's first prune), sorted into m.R by (distance, id) and put through the keep rule, no
// shortcut and no fill; the places the prune emptied are zeroed.  Returns the prunes run.
template <typename VT>
__device__ __forceinline__ uint32_t hnsw_sparse_reverse_group(const HnswSparseBuildArgs &s, const HnswSparseBuildLds &m, const uint64_t *req,
                                                              uint64_t j0, uint64_t jend, int lane) {
  const HnswBuildArgs &b = s.b;
  const HnswArgs &a = b.g;
  const uint64_t head = hnsw_uni64(req[j0]) >> HNSW_REQ_SRC_BITS;
  const uint32_t l = (uint32_t)(head >> 32), t = (uint32_t)head;
  const uint32_t cap = l == 0 ? a.m0 : a.m;
  uint32_t *lcnt;
  uint32_t *lst = hnsw_sparse_own_list(b, l, t, lcnt);
  uint32_t cnt = hnsw_uni(*lcnt), nprune = 0;
  bool have_row = false;
  HnswSparseScorer<VT> to_t{};
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
      to_t = hnsw_sparse_stage_row<VT>(s, m, m.run_a, t, lane);
      have_row = true;
    }
    uint32_t ssize = 0;
    for (uint32_t c0 = 0; c0 < cap + 1; c0 += 64) {
      const uint32_t nc = min(64u, cap + 1 - c0);
      if ((uint32_t)lane < nc) m.coll[lane] = c0 + (uint32_t)lane < cap ? lst[c0 + lane] : src;
      hnsw_sync(false);
      to_t(a, m.coll, m.cdist, nc, lane);
      for (uint32_t jj = 0; jj < nc; ++jj) {
        const uint64_t word = hnsw_pack(__builtin_bit_cast(float, hnsw_uni(__builtin_bit_cast(uint32_t, m.cdist[jj]))), hnsw_uni(m.coll[jj]));
        ssize = hnsw_put(m.R, ssize, cap + 1, word, lane, false);
      }
      hnsw_sync(false);
    }
    uint32_t unused = 0;
    const uint32_t nk = hnsw_sparse_keep<VT>(s, m, m.R, ssize, cap, nullptr, unused, lane);
    for (uint32_t x = (uint32_t)lane; x < cap; x += 64) lst[x] = x < nk ? m.kept[x] : 0u;
    cnt = nk;
    ++nprune;
    hnsw_sync(true);
  }
  if (lane == 0) *lcnt = cnt;
  return nprune;
}

// One wave per (level, target) group of the sorted round buffer, grid-stride; no two waves touch one list (hnsw_reverse_kernel).
template <typename VT>
__global__ __launch_bounds__(64) void hnsw_sparse_reverse_kernel(HnswSparseBuildArgs s, const uint64_t *req, uint64_t slots, const uint32_t *gstart,
                                                                 const uint32_t *ngroups) {
  extern __shared__ f32x4 zvk_smem4[];
  const int lane = (int)threadIdx.x;
  const HnswSparseBuildLds m(reinterpret_cast<unsigned char *>(zvk_smem4), hnsw_sparse_run_bytes(s.run_elems, sizeof(VT)), HNSW_BUILD_MAX_M0 + 2,
                             false);
  const uint32_t ng = hnsw_uni(*ngroups);
  uint32_t nprune = 0;
  for (uint32_t g = blockIdx.x; g < ng; g += gridDim.x) nprune += hnsw_sparse_reverse_group<VT>(s, m, req, hnsw_uni(gstart[g]), slots, lane);
  if (lane == 0 && nprune != 0) atomicAdd(&s.b.counters[2], (unsigned long long)nprune);
}

// The reverse phase of a round of ONE node, on the round buffer as the insert kernel left it: every used word is a whole group
// (hnsw_reverse_one_kernel); one wave per request slot, grid-stride.
template <typename VT>
__global__ __launch_bounds__(64) void hnsw_sparse_reverse_one_kernel(HnswSparseBuildArgs s, uint64_t slots) {
  extern __shared__ f32x4 zvk_smem4[];
  const int lane = (int)threadIdx.x;
  const HnswSparseBuildLds m(reinterpret_cast<unsigned char *>(zvk_smem4), hnsw_sparse_run_bytes(s.run_elems, sizeof(VT)), HNSW_BUILD_MAX_M0 + 2,
                             false);
  uint32_t nprune = 0;
  for (uint64_t j = blockIdx.x; j < slots; j += gridDim.x) {
    if (hnsw_uni64(s.b.req[j]) == HNSW_REQ_NONE) continue;
    nprune += hnsw_sparse_reverse_group<VT>(s, m, s.b.req, j, j + 1, lane);
  }
  if (lane == 0 && nprune != 0) atomicAdd(&s.b.counters[2], (unsigned long long)nprune);
}

}  // namespace zvk
