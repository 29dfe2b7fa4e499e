// zvk_hamming_ivf.hip.h — binary rows under the Hamming metric through inverted lists: probe selection, the list-major plan,
// the list scan, and the k-means step of the trainer (bitwise majority).
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Reference: IVFStreamer::search_impl (src/core/algorithm/ivf/ivf_streamer.cc:183-250) never looks at the data type; its
// IVFCentroidIndex is a flat index over the centroids under the rows' own metric, whose heap admits with a strict `<` (heap.h:103-114),
// so among equal distances the centroid seen first — the lower index — wins.  The trainer's binary branch is
// BinaryKmeansAlgorithm<uint32_t / uint64_t> (src/core/algorithm/cluster/opt_kmeans_cluster.cc:760-851, 1319-1326) over
// BinaryVectorMean (src/core/algorithm/cluster/vector_mean.h:538-650): a centroid is the bitwise majority of its members.
//
// Layout.  The rows live in an ordinary binary Store (zvk_hamming.hip.h) in list order with no padding between the lists: storage
// position == list-order position, list l owns positions [list_off[l], list_off[l + 1]).  A list therefore starts and ends anywhere
// inside a 128-row tile; a boundary tile is shared by two lists and read by both, each masking the other's lanes.  The centroids are
// a second binary Store.
#pragma once
#include "zvk_hamming.hip.h"
#include "zvk_plan.hip.h"

namespace zvk {

// The tiles of the list [lo, hi) (hi > lo) and their cut into at most `nsplit` runs of `tps` tiles: t0 the first tile, nt how many the
// list touches, ns the runs that hold a tile.  The plan and the scan both call this; nothing else decides the cut.
struct BivfListCut {
  uint32_t t0, nt, tps, ns;
};
__host__ __device__ inline BivfListCut bivf_list_cut(uint32_t lo, uint32_t hi, uint32_t nsplit) {
  BivfListCut c;
  c.t0 = lo >> 7;
  c.nt = ((hi - 1) >> 7) - c.t0 + 1;
  c.tps = (c.nt + nsplit - 1) / nsplit;
  c.ns = (c.nt + c.tps - 1) / c.tps;
  return c;
}

// ---- probe selection ----------------------------------------------------------------------------------------------------------
struct BivfSelectArgs {
  const float *dump;              // [nq][dump_stride] exact centroid distances (hamming_scan_kernel<., DUMP>)
  uint32_t dump_stride;
  uint32_t nq, nlist, np;         // np = min(nprobe, nlist) > 0
  uint32_t max_scan_count;
  const uint32_t *list_off;       // [nlist + 1]; nullptr: labelling (no cut, no statistics, no histogram)
  uint32_t *probe_idx;            // [nq][np] centroids ascending by (distance, index)
  uint32_t *probe_cnt;            // [nq] lists probed under the max-scan rule
  uint32_t *scanned;              // [nq] rows of those lists
  uint32_t *list_count;           // [nlist] += queries that probe the (non-empty) list: the histogram of the plan's counting sort
};

// One wave per query.  The key of centroid i is (uint64) distance << 32 | i: unique, so the np smallest in ascending order are one
// well-defined sequence, whatever the scan left free among equal distances.  Rank r is the smallest key above rank r - 1's (every
// lane takes the minimum over its strided share of the row, the wave reduces).  The same walk applies the probe rule of
// IVFStreamer::search_impl (ivf_streamer.cc:223-237): list r is probed while the rows of the lists before it stay below
// max_scan_count, and adds its whole length (an empty list is probed and adds nothing) — what plan_wave_kernel counts for the fp lists.
__global__ void __launch_bounds__(256) bivf_probe_select_kernel(const BivfSelectArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  const float *row = a.dump + (size_t)q * a.dump_stride;
  uint64_t lower = 0;                                   // keys below it are taken
  uint32_t before = 0, probes = 0, rows = 0;            // uniform
  for (uint32_t r = 0; r < a.np; ++r) {
    uint64_t best = ~0ull;
    for (uint32_t i = lane; i < a.nlist; i += 64) {
      const uint64_t key = ((uint64_t)(uint32_t)row[i] << 32) | i;
      if (key >= lower && key < best) best = key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor((unsigned long long)best, off);
      best = o < best ? o : best;
    }
    const uint32_t l = (uint32_t)best;                  // (np <= nlist: a key is always left)
    lower = best + 1;
    if (lane == 0) a.probe_idx[(size_t)q * a.np + r] = l;
    if (a.list_off) {
      const uint32_t len = a.list_off[l + 1] - a.list_off[l];
      if (before < a.max_scan_count) {
        ++probes;
        rows += len;
        if (len && lane == 0) atomicAdd(&a.list_count[l], 1u);
      }
      before += len;
    }
  }
  if (a.list_off && lane == 0) {
    a.probe_cnt[q] = probes;
    a.scanned[q] = rows;
  }
}

// ---- plan: list-major work items by a counting sort (histogram: above; prefix sums: u32_exclusive_scan_kernel; scatter) ---------
struct BivfPlanArgs {
  const uint32_t *probe_idx, *probe_cnt;
  uint32_t nq, np, nlist, nsplit;
  const uint32_t *list_off;       // [nlist + 1]
  const uint32_t *list_count;     // [nlist] the histogram
  uint32_t *list_items;           // [nlist] work items of the list: query blocks x tile runs
  uint32_t *list_fill;            // [nlist] scatter cursors (zeroed before)
  const uint32_t *list_qoff;      // [nlist + 1] prefix sums of list_count
  uint32_t *csr_q, *csr_slot;     // [list_qoff[nlist]] the queries of every list and the first slot of their partial lists
};

__global__ void __launch_bounds__(256) bivf_plan_items_kernel(const BivfPlanArgs p) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= p.nlist) return;
  const uint32_t c = p.list_count[l];
  p.list_items[l] = c ? (c + HAM_QB - 1) / HAM_QB * bivf_list_cut(p.list_off[l], p.list_off[l + 1], p.nsplit).ns : 0u;
}

// one thread per (query, probe rank): the pair joins its list's run of the CSR.  Slot of a partial list: (query * np + rank) * nsplit
// + tile run, so that the slots of a query are contiguous and in probe order (merge_kernel's partial-list shape).
__global__ void __launch_bounds__(256) bivf_plan_scatter_kernel(const BivfPlanArgs p) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (uint64_t)p.nq * p.np) return;
  const uint32_t q = (uint32_t)(w / p.np), r = (uint32_t)(w - (uint64_t)q * p.np);
  if (r >= p.probe_cnt[q]) return;
  const uint32_t l = p.probe_idx[w];
  if (p.list_off[l + 1] == p.list_off[l]) return;
  const uint32_t e = p.list_qoff[l] + atomicAdd(&p.list_fill[l], 1u);
  p.csr_q[e] = q;
  p.csr_slot[e] = (uint32_t)w * p.nsplit;
}

// slots no item writes (ranks past the max-scan cut, empty lists, tile runs a short list does not have) hold +inf / IDX_NONE
__global__ void __launch_bounds__(256) bivf_fill_partials_kernel(float *part_s, uint32_t *part_i, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    part_s[i] = __builtin_inff();
    part_i[i] = IDX_NONE;
  }
}

// ---- list scan ----------------------------------------------------------------------------------------------------------------
struct HamListScanArgs {
  const uint32_t *base;           // blocked binary rows in list order
  const uint32_t *exclude;        // nullable bitset over positions, set = skip
  const uint32_t *queries;        // [nq][cpr * 4] words, zero padded
  uint32_t cpr, k;
  float threshold;
  uint32_t nlist, nsplit;
  const uint32_t *list_off;       // [nlist + 1]
  const uint32_t *list_qoff;      // [nlist + 1]
  const uint32_t *item_off;       // [nlist + 1] prefix sums of list_items; item_off[nlist] = the items of this search
  const uint32_t *csr_q, *csr_slot;
  uint32_t *gtau;                 // [nq] shared bounds, as HamScanArgs::gtau
  float *part_s;                  // [nq][np * nsplit][k]
  uint32_t *part_i;
};

// One wave per work-group, structured like hamming_scan_kernel; item = (list, run of its tiles, block of up to HAM_QB of the queries
// that probe it).  The launch covers an upper bound of the items (the host does not wait for the plan): the work-groups beyond
// item_off[nlist] leave at once.  Lane j of `qn` / `qv` / `sv` holds the number, the first chunk and the slot of the item's j-th
// query; a v_readlane with the loop's constant j makes them scalars, so the query words still arrive as scalar loads.  Lanes whose position
// lies outside [list_lo, list_hi) score +inf: the boundary tiles belong to two lists.
template <bool EXCL>
__global__ void __launch_bounds__(64) hamming_list_scan_kernel(const HamListScanArgs a) {
  extern __shared__ f32x4 zvk_smem4[];
  float *tau = reinterpret_cast<float *>(zvk_smem4);                // [QB] k-th score of a full list, +inf before
  uint32_t *cnt = reinterpret_cast<uint32_t *>(tau + HAM_QB);       // [QB]
  float *gt = reinterpret_cast<float *>(cnt + HAM_QB);              // [QB] shared bound as of this tile
  float *Ls = gt + HAM_QB;                                          // [QB][k]
  uint32_t *Li = reinterpret_cast<uint32_t *>(Ls + (size_t)HAM_QB * a.k);
  const int lane = threadIdx.x;
  const uint32_t item = blockIdx.x;
  if (item >= a.item_off[a.nlist]) return;
  uint32_t l = 0, lend = a.nlist;                                   // item_off[l] <= item < item_off[lend]
  while (lend - l > 1) {
    const uint32_t mid = (l + lend) >> 1;
    if (a.item_off[mid] <= item) l = mid; else lend = mid;
  }
  const uint32_t plo = a.list_off[l], phi = a.list_off[l + 1];      // (a list with items has rows)
  const BivfListCut cut = bivf_list_cut(plo, phi, a.nsplit);
  const uint32_t r = item - a.item_off[l], qb = r / cut.ns, split = r - qb * cut.ns;
  const uint32_t e0 = a.list_qoff[l] + qb * HAM_QB, nqb = min((uint32_t)HAM_QB, a.list_qoff[l + 1] - e0);
  const uint32_t t0 = cut.t0 + split * cut.tps, t1 = min(cut.t0 + cut.nt, t0 + cut.tps);
  const uint32_t k = a.k, cpr = a.cpr;
  uint32_t qn = 0, sv = 0;
  if ((uint32_t)lane < nqb) { qn = a.csr_q[e0 + lane]; sv = a.csr_slot[e0 + lane] + split; }
  const uint32_t qv = qn * cpr;                                     // (the host keeps a slice's query matrix below 2^32 chunks)
  // (uniform values that live in vector registers, of which there are plenty: the list's bounds — a position is inside iff
  // pos - lo < length, unsigned — and the threshold)
  uint32_t vlo = plo, vlen = phi - plo;
  float vthr = a.threshold;
  asm volatile("" : "+v"(vlo), "+v"(vlen), "+v"(vthr));
  const ham_qptr qp = (ham_qptr)(uintptr_t)a.queries;
  if (lane < HAM_QB) { tau[lane] = __builtin_inff(); cnt[lane] = 0; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t *tile = a.base + (size_t)t * cpr * (TILE_N * 4);
    uint32_t nqt = nqb, jz = 0;                                     // (opaque per tile, as in hamming_scan_kernel)
    asm volatile("" : "+s"(nqt), "+s"(jz));
    uint32_t acc[HAM_QB][2];
#pragma unroll
    for (int j = 0; j < HAM_QB; ++j) { acc[j][0] = 0; acc[j][1] = 0; }
    uint32_t c = 0;
    for (; c + 4 <= cpr; c += 4) ham_accumulate<4, true>(tile, qp, cpr, c, nqb, lane, acc, qv);
    if (c + 2 <= cpr) { ham_accumulate<2, true>(tile, qp, cpr, c, nqb, lane, acc, qv); c += 2; }
    if (c < cpr) ham_accumulate<1, true>(tile, qp, cpr, c, nqb, lane, acc, qv);
    const uint32_t p0 = t * TILE_N + lane, p1 = p0 + 64;
    bool ok0 = p0 - vlo < vlen, ok1 = p1 - vlo < vlen;
    if (EXCL) {
      if (ok0) ok0 = ((a.exclude[p0 >> 5] >> (p0 & 31)) & 1u) == 0;
      if (ok1) ok1 = ((a.exclude[p1 >> 5] >> (p1 & 31)) & 1u) == 0;
    }
    // the bounds the work-groups of these queries have published so far
    if ((uint32_t)lane < nqb) gt[lane] = fkey_inv(a.gtau[qn]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < HAM_QB; ++j) {
      if ((uint32_t)j < nqt) {
        const float s0 = ok0 ? (float)acc[j][0] : __builtin_inff(), s1 = ok1 ? (float)acc[j][1] : __builtin_inff();
        const float tg = gt[j];
        float tl = tau[j];
        float b = fminf(tl, tg);
        uint64_t m0 = __ballot(s0 <= vthr && s0 < b), m1 = __ballot(s1 <= vthr && s1 < b);
        if ((m0 | m1) == 0) continue;
        uint32_t n_in = cnt[j];
        float *L = Ls + (size_t)(jz + j) * k;
        uint32_t *I = Li + (size_t)(jz + j) * k;
        bool improved = false;
        while ((m0 | m1) != 0) {
          int ln;
          float cs;
          uint32_t ci;
          if (m0 != 0) {
            ln = __builtin_ctzll(m0);
            cs = bcast_f(s0, ln);
            ci = bcast_u(p0, ln);
            m0 &= m0 - 1;
          } else {
            ln = __builtin_ctzll(m1);
            cs = bcast_f(s1, ln);
            ci = bcast_u(p1, ln);
            m1 &= m1 - 1;
          }
          if (sorted_insert<false>(L, nullptr, I, k, n_in, cs, 0u, ci, lane, tl)) {
            if (n_in == k) {
              improved = true;
              b = fminf(tl, tg);
              m0 &= __ballot(s0 < b);
              m1 &= __ballot(s1 < b);
            }
          }
        }
        const uint32_t qj = bcast_u(qn, j);
        if (lane == 0) {
          cnt[j] = n_in;
          tau[j] = tl;
          if (improved && tl < tg) atomicMin(&a.gtau[qj], fkey(tl));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = 0; j < nqb; ++j) {
    const size_t slot = bcast_u(sv, (int)j);
    const uint32_t c = cnt[j];
    for (uint32_t e = lane; e < k; e += 64) {
      a.part_s[slot * k + e] = e < c ? Ls[(size_t)j * k + e] : __builtin_inff();
      a.part_i[slot * k + e] = e < c ? Li[(size_t)j * k + e] : IDX_NONE;
    }
  }
}

// ---- training: one k-means step on bits -----------------------------------------------------------------------------------------
// plain rows src[idx[c]] -> dst[c] (the initial centroids); one thread per word
__global__ void __launch_bounds__(256) bivf_gather_rows_kernel(const uint32_t *src, const uint64_t *idx, uint32_t n, uint32_t words, uint32_t *dst) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (uint64_t)n * words) return;
  const uint32_t c = (uint32_t)(w / words), e = (uint32_t)(w - (uint64_t)c * words);
  dst[w] = src[(size_t)idx[c] * words + e];
}

// ones[label][bit] += 1 for every set bit of every row, members[label] += 1.  One wave per row at a time, lane = bit of a 64-bit
// group: a wave's atomics fall on 256 contiguous bytes of the row's list.  (BinaryVectorMean::plus, vector_mean.h:582-596)
__global__ void __launch_bounds__(256) bivf_bit_count_kernel(const uint32_t *rows, const uint32_t *labels, uint64_t n, uint32_t words,
                                                             uint32_t *ones, uint32_t *members) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t dim = words * 32;
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (uint64_t)gridDim.x * 4) {
    const uint32_t l = labels[row];
    const uint32_t *src = rows + (size_t)row * words;
    for (uint32_t b = lane; b < dim; b += 64)
      if ((src[b >> 5] >> (b & 31)) & 1u) atomicAdd(&ones[(size_t)l * dim + b], 1u);
    if (lane == 0) atomicAdd(&members[l], 1u);
  }
}

// bit i of a centroid with members is set iff ones_i > (members >> 1) (BinaryVectorMean::mean, vector_mean.h:599-613); a centroid
// without members keeps its bits.  One thread per centroid word.
__global__ void __launch_bounds__(256) bivf_majority_kernel(const uint32_t *ones, const uint32_t *members, uint32_t nlist, uint32_t words,
                                                            uint32_t *cent) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (uint64_t)nlist * words) return;
  const uint32_t l = (uint32_t)(w / words), e = (uint32_t)(w - (uint64_t)l * words);
  const uint32_t m = members[l];
  if (m == 0) return;
  const uint32_t *o = ones + ((size_t)l * words + e) * 32;
  uint32_t bits = 0;
#pragma unroll
  for (int b = 0; b < 32; ++b) bits |= (o[b] > (m >> 1) ? 1u : 0u) << b;
  cent[w] = bits;
}

}  // namespace zvk
