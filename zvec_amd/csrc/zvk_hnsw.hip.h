// zvk_hnsw.hip.h — batched beam search on a built HNSW graph (zvec_hip_hnsw_*, api_entry_hnsw.inc.h): one wave per query walks the
// graph by the rule of DESIGN §3c, which restates HnswAlgorithm::search, select_entry_point and search_neighbors
// (hnsw_algorithm.cc:83-278).  The walk is latency- and gather-bound: nothing here touches the matrix cores.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// A (distance, node) pair is ONE 64-bit word, fkey(distance) in the high half and the node id in the low half, so that the order
// "ascending by (distance, node id)" is the order of the words.  The result list R (at most ef <= 512 words) and the candidate set C
// are arrays of such words sorted ascending.  R lives in LDS.  C starts in LDS (HNSW_C_LDS words) and moves, once, into the query's
// region of the context workspace when more than that many candidates are alive at the same time (rows excluded by the caller's
// bitset are traversed but never fill R, so nothing bounds C below the row count then).
//
// Rows and queries are fp32 or IEEE binary16 (template parameter H of everything that touches their memory: H = true, halves).  A half
// is widened to fp32 where it is read, which is exact (subnormals included, nothing flushed); from there on the arithmetic is the
// fp32 kernel's own, operation for operation and in the same order, so an fp16 handle answers bit for bit as an fp32 handle given the
// widened values would (DESIGN §3c "fp16 rows").  LDS holds the query, and the build's candidate row, as fp32 either way.
#pragma once
#include "zvk_common.hip.h"

namespace zvk {

constexpr uint32_t HNSW_MAX_EF = 512;      // words of R: 4 KiB of LDS per query
constexpr uint32_t HNSW_C_LDS = 1024;      // words of C held in LDS: 8 KiB per query
constexpr uint32_t HNSW_MAX_DIM = 4096;    // the query row is kept in LDS

struct HnswArgs {
  const void *rows;           // [n][dpad] row-major, zero padded; dpad is a multiple of 4 elements (a lane loads 16 bytes of
                              // fp32, 8 bytes of fp16: the same four elements; an fp16 row is 8-byte aligned and no more)
  const uint64_t *keys;       // [n]
  const uint32_t *nbr0;       // [n][m0]
  const uint32_t *cnt0;       // [n]
  const uint32_t *upper_of;   // [n] index into the upper table, IDX_NONE = level 0 only
  const uint32_t *nbr_up;     // [n_upper][max_level][m]
  const uint32_t *cnt_up;     // [n_upper][max_level]
  uint32_t n, dim, dpad, m0, m, max_level, entry;
  int ip;                     // 0: squared L2, 1: minus the dot product
  const void *queries;        // [nq][dim], the rows' element type
  const uint32_t *exclude;    // nullable, 1 bit per position
  uint32_t topk, ef, max_scan;
  float threshold;
  uint32_t *visited;          // [nq][vis_words], zero on entry
  uint32_t vis_words;
  uint64_t *cand_ws;          // [nq][ccap] when ccap > HNSW_C_LDS, else null
  uint32_t ccap;              // capacity of C: min(max_scan, n)
  uint64_t *out_keys;         // [nq][topk]
  float *out_scores;          // [nq][topk]
  uint32_t *out_counts;       // [nq]
  uint32_t *stats;            // [nq][2]: distances computed, nodes expanded
};

__host__ __device__ inline size_t hnsw_lds_bytes(uint32_t dpad, uint32_t ef) {
  return (size_t)dpad * 4 + (size_t)ef * 8 + (size_t)HNSW_C_LDS * 8 + 64 * 4 + 64 * 4;
}

// what differs between the two element types: the element itself, and the four elements a lane loads per step
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <bool H> struct HnswElem { typedef float type; typedef f32x4 step; };
template <> struct HnswElem<true> { typedef _Float16 type; typedef f16x4 step; };
__device__ __forceinline__ f32x4 hnsw_widen(f32x4 v) { return v; }
__device__ __forceinline__ f32x4 hnsw_widen(f16x4 v) { return __builtin_convertvector(v, f32x4); }
// element i of an array of rows or queries, as fp32
template <bool H>
__device__ __forceinline__ float hnsw_elem(const void *p, size_t i) { return (float)static_cast<const typename HnswElem<H>::type *>(p)[i]; }

// what one lane wrote to LDS (or, glob, to the query's workspace region) is visible to the other lanes of its wave afterwards
__device__ __forceinline__ void hnsw_sync(bool glob) {
  if (glob) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t hnsw_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t hnsw_uni64(uint64_t v) { return ((uint64_t)hnsw_uni((uint32_t)(v >> 32)) << 32) | hnsw_uni((uint32_t)v); }

__device__ __forceinline__ uint64_t hnsw_pack(float d, uint32_t id) {
  if (__builtin_bit_cast(uint32_t, d) == 0x80000000u) d = 0.f;       // (-0 and +0 are one distance)
  return ((uint64_t)fkey(d) << 32) | id;
}

// Whole-wave insertion of word v into the ascending array A of `size` words with room for `cap`: the words behind its place move
// up by one; in a full array the largest word leaves, which may be v itself.  Returns the new size.
__device__ __forceinline__ uint32_t hnsw_put(uint64_t *A, uint32_t size, uint32_t cap, uint64_t v, int lane, bool glob) {
  uint32_t end = size;
  if (size == cap) {
    if (hnsw_uni64(A[cap - 1]) < v) return size;
    end = cap - 1;
  }
  uint32_t p = 0;
  for (uint32_t j0 = 0; j0 < end; j0 += 64) {
    const uint32_t j = j0 + (uint32_t)lane;
    const bool less = j < end && A[j] < v;
    const uint32_t c = (uint32_t)__popcll(__ballot(less));
    p += c;
    if (c < 64) break;                                   // (ascending: nothing further on is smaller)
  }
  if (end > p) {
    for (int mm = (int)((end - 1) >> 6); mm >= (int)(p >> 6); --mm) {      // top chunk first: never overwrites unread words
      const uint32_t j = (uint32_t)mm * 64u + (uint32_t)lane;
      const bool mv = j >= p && j < end;
      uint64_t t = 0;
      if (mv) t = A[j];
      hnsw_sync(glob);
      if (mv) A[j + 1] = t;
      hnsw_sync(glob);
    }
  }
  if (lane == 0) A[p] = v;
  hnsw_sync(glob);
  return end + 1;
}

// cdist[r] = the score of row coll[r] for r < nc (nc <= 64).  Sixteen lanes take a row, four elements each per step (16 bytes of
// fp32, 8 bytes of fp16), four rows in flight per wave; the first step of the next four rows is requested before the current four are
// reduced across their lanes.  Element e is component e % 4 of lane (e / 4) % 16 under either type: one summation order.
template <bool H>
__device__ __forceinline__ void hnsw_distances(const HnswArgs &a, const float *qv, const uint32_t *coll, float *cdist, uint32_t nc, int lane) {
  const uint32_t grp = (uint32_t)lane >> 4, sub = (uint32_t)lane & 15u;
  const uint32_t nv = a.dpad >> 2;
  const f32x4 *q4 = reinterpret_cast<const f32x4 *>(qv);
  typedef typename HnswElem<H>::step step;
  const step *rows4 = static_cast<const step *>(a.rows);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  uint32_t r = grp;
  const step *row = rows4 + (size_t)coll[r < nc ? r : 0] * nv;
  f32x4 b0 = sub < nv ? hnsw_widen(row[sub]) : zero;
  for (uint32_t g = 0; g < nc; g += 4) {
    f32x4 acc = zero;
    if (sub < nv) {
      const f32x4 x = q4[sub];
      if (a.ip) acc = b0 * x;
      else { const f32x4 d = x - b0; acc = d * d; }
    }
#pragma unroll 4
    for (uint32_t t = sub + 16; t < nv; t += 16) {
      const f32x4 b = hnsw_widen(row[t]), x = q4[t];
      if (a.ip) {
        acc.x = fmaf(b.x, x.x, acc.x); acc.y = fmaf(b.y, x.y, acc.y); acc.z = fmaf(b.z, x.z, acc.z); acc.w = fmaf(b.w, x.w, acc.w);
      } else {
        const f32x4 d = x - b;
        acc.x = fmaf(d.x, d.x, acc.x); acc.y = fmaf(d.y, d.y, acc.y); acc.z = fmaf(d.z, d.z, acc.z); acc.w = fmaf(d.w, d.w, acc.w);
      }
    }
    const uint32_t rcur = r;
    r += 4;
    row = rows4 + (size_t)coll[r < nc ? r : 0] * nv;
    if (g + 4 < nc) b0 = sub < nv ? hnsw_widen(row[sub]) : zero;     // the next rows' first loads go out before the reduction below
    float s = (acc.x + acc.y) + (acc.z + acc.w);
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    if (sub == 0 && rcur < nc) cdist[rcur] = a.ip ? -s : s;
  }
  hnsw_sync(false);
}

__device__ __forceinline__ bool hnsw_excluded(const HnswArgs &a, uint32_t id) {
  return a.exclude != nullptr && ((a.exclude[id >> 5] >> (id & 31u)) & 1u) != 0;
}

// the list of node c on level l: level 0 is nbr0 / cnt0, level l >= 1 is slot l - 1 of c's place in the upper table
__device__ __forceinline__ const uint32_t *hnsw_list(const HnswArgs &a, uint32_t l, uint32_t c, uint32_t &cnt) {
  if (l == 0) {
    cnt = hnsw_uni(a.cnt0[c]);
    return a.nbr0 + (size_t)c * a.m0;
  }
  const size_t slot = (size_t)hnsw_uni(a.upper_of[c]) * a.max_level + (l - 1);
  cnt = hnsw_uni(a.cnt_up[slot]);
  return a.nbr_up + slot * a.m;
}

// step 2 of the rule on level l >= 1: greedy, no visited set, no scan limit; moves ep / dist
template <bool H>
__device__ __forceinline__ void hnsw_greedy(const HnswArgs &a, uint32_t l, const float *qv, uint32_t *coll, float *cdist, uint32_t &ep,
                                            float &dist, uint32_t &scanned, int lane) {
  bool changed = true;
  while (changed) {
    changed = false;
    uint32_t cnt;
    const uint32_t *lst = hnsw_list(a, l, ep, cnt);
    for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
      const uint32_t nc = min(64u, cnt - c0);
      uint32_t id = 0;
      if ((uint32_t)lane < nc) { id = lst[c0 + lane]; coll[lane] = id; }
      hnsw_sync(false);
      hnsw_distances<H>(a, qv, coll, cdist, nc, lane);
      scanned += nc;
      const float d = (uint32_t)lane < nc ? cdist[lane] : __builtin_inff();
      float mn = d;
      for (int o = 32; o >= 1; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
      if (mn < dist) {                                   // stored order, strict: the first row at the pass's smallest distance
        const uint64_t at = __ballot((uint32_t)lane < nc && d == mn);
        if (at != 0) {
          dist = mn;
          ep = bcast_u(id, __builtin_ctzll(at));
          changed = true;
        }
      }
      hnsw_sync(false);
    }
  }
}

// step 3 of the rule on level l from ep (at distance dist): fills R (capacity a.ef, ascending) and returns its size.  C is the
// HNSW_C_LDS words in LDS, G the walk's region of a.ccap words in the workspace (null when a.ccap fits LDS); vis is the walk's
// visited bits, zero on entry.  The search kernel calls it on level 0, the build (zvk_hnsw_build.hip.h) on every level.
template <bool H>
__device__ __forceinline__ uint32_t hnsw_beam(const HnswArgs &a, uint32_t l, const float *qv, uint64_t *R, uint64_t *C, uint64_t *G,
                                              uint32_t *coll, float *cdist, uint32_t *vis, uint32_t ep, float dist, uint32_t &scanned,
                                              uint32_t &hops, int lane) {
  if (lane == 0) atomicOr(&vis[ep >> 5], 1u << (ep & 31u));
  uint32_t rsize = 0, csize = 1, chead = 0, cbuf = min(HNSW_C_LDS, a.ccap);
  bool cglob = false;
  {
    const uint64_t w = hnsw_pack(dist, ep);
    if (!hnsw_excluded(a, ep)) { if (lane == 0) R[0] = w; rsize = 1; }
    if (lane == 0) C[0] = w;
  }
  hnsw_sync(false);
  while (csize > 0 && scanned < a.max_scan) {
    const uint64_t top = hnsw_uni64(C[chead]);
    if (rsize == a.ef && (uint32_t)(top >> 32) > (uint32_t)(hnsw_uni64(R[a.ef - 1]) >> 32)) break;
    ++chead; --csize; ++hops;
    uint32_t cnt;
    const uint32_t *lst = hnsw_list(a, l, (uint32_t)top, cnt);
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
      hnsw_distances<H>(a, qv, coll, cdist, nc, lane);
      scanned += nc;
      // a row that fails `distance < worst(R)` against a full R fails it for good (the worst of a full R never grows): skip those
      uint64_t todo = nc == 64 ? ~0ull : ((1ull << nc) - 1ull);
      if (rsize == a.ef) {
        const uint32_t worst = (uint32_t)(hnsw_uni64(R[a.ef - 1]) >> 32);
        todo = __ballot((uint32_t)lane < nc && fkey(cdist[lane]) < worst);
      }
      while (todo != 0) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t idj = hnsw_uni(coll[j]);
        const uint64_t w = hnsw_pack(__builtin_bit_cast(float, hnsw_uni(__builtin_bit_cast(uint32_t, cdist[j]))), idj);
        if (rsize == a.ef && !((uint32_t)(w >> 32) < (uint32_t)(hnsw_uni64(R[a.ef - 1]) >> 32))) continue;
        // into C: make room at the end of the buffer first
        if (chead + csize == cbuf) {
          if (chead > 0) {                               // slide the words down to the start of the buffer
            for (uint32_t j0 = 0; j0 < csize; j0 += 64) {
              const uint32_t jj = j0 + (uint32_t)lane;
              uint64_t t = 0;
              if (jj < csize) t = C[chead + jj];
              hnsw_sync(cglob);
              if (jj < csize) C[jj] = t;
              hnsw_sync(cglob);
            }
            chead = 0;
          } else if (!cglob && G != nullptr) {           // LDS is full of live candidates: go on in the walk's workspace region
            for (uint32_t jj = (uint32_t)lane; jj < csize; jj += 64) G[jj] = C[jj];
            C = G;
            cbuf = a.ccap;
            cglob = true;
            hnsw_sync(true);
          }
        }
        csize = hnsw_put(C + chead, csize, cbuf - chead, w, lane, cglob);
        if (!hnsw_excluded(a, idj)) rsize = hnsw_put(R, rsize, a.ef, w, lane, false);
      }
      hnsw_sync(false);
    }
    // candidates beyond the worst of a full R can never be popped: they leave now (DESIGN §3c argues that nothing observable changes)
    if (rsize == a.ef) {
      const uint32_t worst = (uint32_t)(hnsw_uni64(R[a.ef - 1]) >> 32);
      while (csize > 0 && (uint32_t)(hnsw_uni64(C[chead + csize - 1]) >> 32) > worst) --csize;
    }
  }
  return rsize;
}

template <bool H>
__global__ __launch_bounds__(64) void hnsw_search_kernel(HnswArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_smem[];
  const int lane = (int)threadIdx.x;
  const uint32_t q = blockIdx.x;
  float *qv = reinterpret_cast<float *>(hnsw_smem);
  uint64_t *R = reinterpret_cast<uint64_t *>(qv + a.dpad);
  uint64_t *C = R + a.ef;
  uint32_t *coll = reinterpret_cast<uint32_t *>(C + HNSW_C_LDS);
  float *cdist = reinterpret_cast<float *>(coll + 64);
  for (uint32_t i = (uint32_t)lane; i < a.dpad; i += 64) qv[i] = i < a.dim ? hnsw_elem<H>(a.queries, (size_t)q * a.dim + i) : 0.f;
  if (lane == 0) coll[0] = a.entry;
  hnsw_sync(false);

  // 1. the entry point
  uint32_t scanned = 1, hops = 0, ep = a.entry;
  hnsw_distances<H>(a, qv, coll, cdist, 1, lane);
  float dist = cdist[0];
  hnsw_sync(false);

  // 2. the upper levels
  for (uint32_t l = a.max_level; l >= 1; --l) hnsw_greedy<H>(a, l, qv, coll, cdist, ep, dist, scanned, lane);

  // 3. level 0
  const uint32_t rsize = hnsw_beam<H>(a, 0, qv, R, C, a.cand_ws != nullptr ? a.cand_ws + (size_t)q * a.ccap : nullptr, coll, cdist,
                                   a.visited + (size_t)q * a.vis_words, ep, dist, scanned, hops, lane);

  // 4. the first topk of R within the threshold
  const uint32_t lim = min(a.topk, rsize);
  uint32_t outc = 0;
  for (uint32_t j0 = 0; j0 < a.topk; j0 += 64) {
    const uint32_t j = j0 + (uint32_t)lane;
    bool ok = j < lim;
    uint64_t w = 0;
    float d = 0.f;
    if (ok) {
      w = R[j];
      d = fkey_inv((uint32_t)(w >> 32));
      ok = d <= a.threshold;
    }
    if (j < a.topk) {
      a.out_keys[(size_t)q * a.topk + j] = ok ? a.keys[(uint32_t)w] : ~0ull;
      a.out_scores[(size_t)q * a.topk + j] = ok ? d : __builtin_inff();
    }
    outc += (uint32_t)__popcll(__ballot(ok));
  }
  if (lane == 0) {
    a.out_counts[q] = outc;
    a.stats[2 * (size_t)q] = scanned;
    a.stats[2 * (size_t)q + 1] = hops;
  }
}

// an index without rows: every list is empty and nothing was walked
__global__ void hnsw_empty_kernel(uint64_t *out_keys, float *out_scores, uint32_t *out_counts, uint32_t *stats, uint32_t nq, uint32_t topk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (uint64_t)nq * topk) {
    out_keys[i] = ~0ull;
    out_scores[i] = __builtin_inff();
  }
  if (i < nq) out_counts[i] = 0;
  if (i < 2 * (uint64_t)nq) stats[i] = 0;
}

}  // namespace zvk
