// zvk_sparse.hip.h — sparse fp32 / fp16 rows under InnerProductSparse and SquaredEuclideanSparse: CSR rows in HBM, the query-block scan, listed rows, the wave-per-row score dump, staging and unpack.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Reference: FlatSparseStreamer / FlatSparseSearcher (src/core/algorithm/flat_sparse/flat_sparse_search.h:119-144) score one query
// at a time against every stored row with MinusInnerProductSparseMatrix<float>::Compute (src/ailego/math/inner_product_matrix.h:
// 2781-2862): a merge join of two index runs that are ascending, score = -(sum of value products over shared indices).
//
// Value type (template parameter VT of every kernel below: float or _Float16).  InnerProductSparseMetric::sparse_distance
// (src/core/metric/inner_product_metric.cc:484-495) picks MinusInnerProductSparseMatrix<ailego::Float16>::Compute for DT_FP16 and the
// <float> one for DT_FP32.  The Float16 one (src/ailego/math/inner_product_matrix_fp16.cc:1924-1945) gathers the matched halves of a
// segment (InnerProductSparseInSegmentAVX, :1066-1202), widens them with _mm256_cvtph_ps and accumulates the products in fp32
// (:1208-1223; the scalar form, :1897-1921, sums Float16 * Float16 into a float the same way).  Here every half is widened to fp32
// where it is read (exact, subnormals included), the product is formed and summed in fp32 with fmaf exactly as for fp32 rows: no half
// arithmetic anywhere.  Halves stay halves in HBM and in LDS.
//
// Layout.  Rows are CSR: row_off[n + 1] (u64 element offsets), idx[elements] (u32, strictly ascending inside a row), val[elements]
// (VT), keys[n].  A position is a row number; exclude bits index positions as in the flat store.
//
// Scan.  ONE wave per work-group, lane = query.  A query block is up to 64 consecutive queries whose runs (at most
// SPARSE_IMG_ELEMS elements together, chosen greedily on the host) are copied to LDS as they stand in the CSR query arrays.  The
// wave walks the rows of its chunk; 64 stored elements are fetched by one coalesced load, then each element's (index, value) is
// broadcast (v_readlane) and every lane binary-searches ITS OWN query's run in LDS and accumulates value * q_value: no cross-lane
// reduction, and after a row every lane holds that row's score for its own query.  Four elements are searched at a time (four
// independent chains of dependent LDS reads).  A run of length 0 makes no LDS read at all.  Lists are lane-owned, kept sorted by
// insertion in LDS as [entry][lane] (lane-major: lanes that work on different entries still hit different banks); admission is
// STRICT against min(own k-th score once the list is full, the bound the work-groups of the same query share) — zero scores tie
// massively and a tie at the k-th place is never needed — and the threshold is a separate non-strict test.
//
// Metric (template parameter L2 of the three scoring kernels and of the helpers they share: sparse_match_step, sparse_score,
// sparse_lane_dot, sparse_wave_row_score, sparse_stage_run, sparse_wave_score_rows; false = InnerProductSparse, the code above,
// with no run-time branch on the metric anywhere).  SquaredEuclideanSparse (SquaredEuclideanSparseMetric, src/core/metric/
// euclidean_metric.cc:1027-1095, which hands out SquaredEuclideanSparseDistanceMatrix<float>::Compute, src/ailego/math/
// euclidean_distance_matrix.h:2480-2638, for DT_FP16 as well as DT_FP32, :1070-1072) runs over the UNION of the two index sets: a
// shared index adds (b - q)^2, an index of the row alone b^2, an index of the query alone q^2.  Here the score is s = A + R, all
// fp32, halves widened first:
//   A   over the stored elements of the row, each one fmaf(x, x, A) with x = b - q (rounded once) where the index is in the query's
//       run and x = b where it is not; the same walk counts the hits and sums Mq = the q^2 of the matched query elements
//       (sparse_match_step)
//   R   the query mass that met nothing: exactly +0 if hits == qlen (the empty query included), else max(0, Qn - Mq)
//       (sparse_score), Qn = the sum of q^2 over the whole run, formed ONCE per work item from the LDS image (never per row)
// so identical runs, a pair of empty runs included, score exactly +0.0 (the norm expansion |b|^2 + |q|^2 - 2 b.q cancels exactly
// there and cannot), every term is >= 0 and a score is never -0.  Nothing is skipped for an empty query or a pair without a shared
// index: both are ordinary, non-zero candidates.
#pragma once
#include "zvk_common.hip.h"

namespace zvk {

constexpr uint32_t SPARSE_MAX_COUNT = 4096;    // PARAM_FLAT_SPARSE_MAX_DIM_SIZE (flat_sparse_utility.h:22)
constexpr uint32_t SPARSE_QB = 64;             // queries per query block at most (one lane each)
constexpr uint32_t SPARSE_IMG_ELEMS = 4096;    // elements of a query block's LDS image at most (32 KiB of fp32, 24 KiB of fp16: one longest query fits)
constexpr uint32_t SPARSE_FUSED_MAX_K = 128;   // lane-owned lists: 64 x k x 8 bytes next to the image; longer lists take the dump route

// What every scoring kernel reads: the stored rows, the exclude bits and the queries.  The first member of each argument struct.
struct SparseOperands {
  const uint64_t *row_off;    // [n + 1]
  const uint32_t *idx;        // [elements]
  const void *val;            // [elements] of the kernel's VT
  const uint32_t *exclude;    // nullable bitset over positions, set = skip
  const uint32_t *q_off;      // [nq + 1] element offsets of the queries in q_idx / q_val
  const uint32_t *q_idx;
  const void *q_val;          // VT as well
};

struct SparseScanArgs {
  SparseOperands op;
  const uint32_t *blk;        // [blocks + 1] first query of every query block
  uint32_t blk0;              // first query block of this launch
  uint32_t qsub0;             // DUMP: the query whose scores are row 0 of `dump`
  uint32_t k;
  float threshold;
  uint64_t n;                 // rows
  uint32_t rows_per_chunk;
  uint32_t nchunks;
  uint32_t nqblocks;          // query blocks of this launch
  uint32_t *gtau;             // [nq] shared bounds (fkey of a full list's k-th score; +inf at the start)
  float *dump;                // DUMP: [queries of the sub-batch][n] scores, +inf for excluded positions
  float *part_s;              // [nq][nchunks][k]
  uint32_t *part_i;
};

// lists | image indices (u32) | image values (`width` bytes each: 4 = fp32, 2 = fp16), the values rounded up to whole words
__host__ __device__ inline size_t sparse_lds_bytes(uint32_t img_elems, uint32_t k_lists, uint32_t width) {
  return ((size_t)2 * SPARSE_QB * k_lists + img_elems) * 4 + (((size_t)img_elems * width + 3) & ~(size_t)3) + 16;
}
// the same for ONE run and no lists (sparse_stage_run): indices | values
__host__ __device__ inline size_t sparse_run_lds_bytes(uint32_t run_elems, uint32_t width) {
  return (size_t)run_elems * 4 + (((size_t)run_elems * width + 3) & ~(size_t)3);
}

// One halving of the lower bound of t[u] in a run of the LDS image qi, U independent chains of dependent LDS reads.  n[u] comes in
// as the run's length (0: no read at all) and base[u] as its start; the answer stays inside [base[u], base[u] + n[u]], and after
// as many halvings as take the longest run down to one element (wave-uniform) n[u] is 1 or 0.
template <int U>
__device__ __forceinline__ void sparse_halve(const uint32_t *qi, const uint32_t (&t)[U], uint32_t (&base)[U], uint32_t (&n)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (n[u] > 1) {
      const uint32_t half = n[u] >> 1;
      if (qi[base[u] + half - 1] < t[u]) base[u] += half;
      n[u] -= half;
    }
  }
}

// One stored element (index t, value v) once the halvings have left its lower bound in the run at base (n = 1) or the run is
// empty (n = 0): one equality probe, and
//   not L2  on a hit one fmaf of the value product into acc; mq and hits are left alone
//   L2      every element adds a square to acc, (b - q)^2 on a hit and b^2 otherwise, a run of length 0 included (v = 0 from a
//           lane or an element beyond the row adds +0); a hit adds its q^2 to mq and 1 to hits
template <typename VT, bool L2>
__device__ __forceinline__ void sparse_match_step(const uint32_t *qi, const VT *qv, uint32_t base, uint32_t n, uint32_t t, float v,
                                                  float &acc, float &mq, uint32_t &hits) {
  if constexpr (L2) {
    float x = v;
    if (n != 0) {
      if (qi[base] == t) {
        const float qx = (float)qv[base];
        x = v - qx;
        mq = __builtin_fmaf(qx, qx, mq);
        ++hits;
      }
    }
    acc = __builtin_fmaf(x, x, acc);
  } else {
    if (n != 0) {
      if (qi[base] == t) acc = __builtin_fmaf(v, (float)qv[base], acc);
    }
  }
}

// A row's sums -> its score, smaller is better.  Not L2: MINUS the inner product; no shared index: exactly +0.  L2: A + R, >= +0
// and never -0.
template <bool L2>
__device__ __forceinline__ float sparse_score(float acc, float mq, uint32_t hits, uint32_t qlen, float qn) {
  if constexpr (L2) return acc + (hits == qlen ? 0.f : fmaxf(0.f, qn - mq));
  else return 0.f - acc;
}

// One wave per work-group; item = (chunk of rows, query block).  DUMP: every score goes to the [query][position] matrix and nothing
// is selected (large k, selected by merge_kernel).
template <typename VT, bool EXCL, bool DUMP, bool L2 = false>
__global__ void __launch_bounds__(64) sparse_scan_kernel(const SparseScanArgs a) {
  extern __shared__ f32x4 zvk_smem4[];
  const int lane = threadIdx.x;
  const SparseOperands &o = a.op;
  const VT *val = static_cast<const VT *>(o.val), *q_val = static_cast<const VT *>(o.q_val);
  const uint32_t k = a.k, kl = DUMP ? 0u : k;
  float *Ls = reinterpret_cast<float *>(zvk_smem4);                   // [k][64] lane-owned lists, ascending
  uint32_t *Li = reinterpret_cast<uint32_t *>(Ls + (size_t)SPARSE_QB * kl);
  uint32_t *qi = Li + (size_t)SPARSE_QB * kl;                         // [tot] the block's query indices, run after run
  const uint32_t chunk = blockIdx.x / a.nqblocks, qb = a.blk0 + (blockIdx.x - chunk * a.nqblocks);
  const uint32_t q0 = a.blk[qb], nqb = a.blk[qb + 1] - q0;
  const uint32_t e0 = o.q_off[q0], tot = o.q_off[q0 + nqb] - e0;
  VT *qv = reinterpret_cast<VT *>(qi + tot);                          // [tot] their values, as stored
  for (uint32_t i = lane; i < tot; i += 64) {
    qi[i] = o.q_idx[e0 + i];
    qv[i] = q_val[e0 + i];
  }
  const bool mine = (uint32_t)lane < nqb;
  uint32_t qstart = 0, qlen = 0;
  if (mine) {
    const uint32_t b = o.q_off[q0 + lane];
    qstart = b - e0;
    qlen = o.q_off[q0 + lane + 1] - b;
  }
  // halvings that take the longest run of the block down to one element (wave-uniform)
  uint32_t steps = 0;
  while (__ballot(qlen > (1u << steps)) != 0) ++steps;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // L2: Qn, the squares of the lane's own run, once per work item (a lane-owned walk of the image)
  float qn = 0.f;
  if constexpr (L2) {
    for (uint32_t i = 0; i < qlen; ++i) {
      const float x = (float)qv[qstart + i];
      qn = __builtin_fmaf(x, x, qn);
    }
  }

  uint32_t cnt = 0;                   // entries of this lane's list
  float tl = __builtin_inff();        // its k-th score once it is full
  const uint64_t r0 = (uint64_t)chunk * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint64_t r = r0; r < r1; ++r) {
    if (EXCL) {
      if ((o.exclude[r >> 5] >> (r & 31)) & 1u) {       // (uniform)
        if (DUMP && mine) a.dump[(size_t)(q0 + lane - a.qsub0) * a.n + r] = __builtin_inff();
        continue;
      }
    }
    uint32_t tgk = 0;
    if (!DUMP && mine) tgk = __hip_atomic_load(&a.gtau[q0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t rb = o.row_off[r], re = o.row_off[r + 1];
    float acc = 0.f;
    float mq = 0.f;                   // L2: the squares of the query elements this row matched, and how many
    uint32_t hits = 0;
    for (uint64_t p = rb; p < re; p += 64) {
      const uint32_t m = (uint32_t)min((uint64_t)64, re - p);
      uint32_t ri = 0;
      float rv = 0.f;
      if ((uint32_t)lane < m) {
        ri = o.idx[p + lane];
        rv = (float)val[p + lane];                        // (a half widens exactly)
      }
      for (uint32_t u0 = 0; u0 < m; u0 += 4) {
        uint32_t t[4], base[4], n[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t e = u0 + u;                    // (uniform; the lane read is kept inside the wave for e >= m)
          t[u] = bcast_u(ri, (int)(e & 63));
          v[u] = bcast_f(rv, (int)(e & 63));
          n[u] = e < m ? qlen : 0u;
          base[u] = qstart;
        }
        // lower bound of t in the lane's run [qstart, qstart + qlen): the answer stays inside [base, base + n]
        for (uint32_t s = 0; s < steps; ++s) sparse_halve<4>(qi, t, base, n);
#pragma unroll
        for (int u = 0; u < 4; ++u) sparse_match_step<VT, L2>(qi, qv, base[u], n[u], t[u], v[u], acc, mq, hits);
      }
    }
    const float s = sparse_score<L2>(acc, mq, hits, qlen, qn);
    if (DUMP) {
      if (mine) a.dump[(size_t)(q0 + lane - a.qsub0) * a.n + r] = s;
      continue;
    }
    const float tg = fkey_inv(tgk);
    if (mine && s <= a.threshold && s < fminf(tl, tg)) {
      // the lane's own sorted insertion: entries above s move up by one, the last one of a full list drops out
      uint32_t p = cnt < k ? cnt : k - 1;
      while (p > 0) {
        const float es = Ls[(size_t)(p - 1) * SPARSE_QB + lane];
        if (!(es > s)) break;
        Ls[(size_t)p * SPARSE_QB + lane] = es;
        Li[(size_t)p * SPARSE_QB + lane] = Li[(size_t)(p - 1) * SPARSE_QB + lane];
        --p;
      }
      Ls[(size_t)p * SPARSE_QB + lane] = s;
      Li[(size_t)p * SPARSE_QB + lane] = (uint32_t)r;
      if (cnt < k) ++cnt;
      if (cnt == k) {
        tl = Ls[(size_t)(k - 1) * SPARSE_QB + lane];
        if (tl < tg) atomicMin(&a.gtau[q0 + lane], fkey(tl));
      }
    }
  }
  if (DUMP) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = 0; j < nqb; ++j) {
    const size_t slot = (size_t)(q0 + j) * a.nchunks + chunk;
    const uint32_t c = bcast_u(cnt, (int)j);
    for (uint32_t e = lane; e < k; e += 64) {
      a.part_s[slot * k + e] = e < c ? Ls[(size_t)e * SPARSE_QB + j] : __builtin_inff();
      a.part_i[slot * k + e] = e < c ? Li[(size_t)e * SPARSE_QB + j] : IDX_NONE;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Listed rows (FlatSparseStreamer::search_bf_by_p_keys_impl, flat_sparse_streamer.cc:324-349; FlatSparseEntity::search_p_keys,
// flat_sparse_entity.h:63-77; batch_distance): every query meets a short list of positions, so the parallelism comes from inside a
// row: lane = STORED ELEMENT.  One wave per work-group; a work item is one query and a slice of at most SPARSE_ROWS_SLICE of its
// listed entries.  The query's run is copied to LDS once per item.  The entries of the slice are classified lane = entry (position
// >= n or excluded: skipped before anything of the row is fetched; else the row's two offsets), then the wave takes the live
// entries one after the other (wave-uniform): 64 stored elements per coalesced load, every lane lower-bounds ITS OWN stored index
// in the query's run (ceil(log2(run length)) halvings, wave-uniform trip count, one equality probe, on a hit one fmaf into a
// lane-private sum), and after the row one butterfly adds the 64 sums up.  Rows longer than 64 elements take four loads at a time:
// four independent chains of dependent LDS reads.  Scores leave as one coalesced store per slice into a ragged [entries] array,
// +inf for a skipped entry; merge_kernel selects over each query's slice of it (slot_begin = the list offsets, one candidate per
// slot), so ties are ordered by the place in the list.
constexpr uint32_t SPARSE_ROWS_SLICE = 64;     // listed entries per work item at most (one lane each while they are classified)

struct SparseRowsArgs {
  SparseOperands op;
  const uint32_t *ids;        // [entries] listed positions, query after query; any value (>= n: skipped)
  const uint32_t *list_off;   // [nq + 1] entries of every query
  const uint32_t *item_q;     // [items] the query of a work item
  const uint32_t *item_e0;    // [items] its first entry
  uint32_t slice;             // entries per item at most, <= SPARSE_ROWS_SLICE
  uint64_t n;                 // rows
  float *scores;              // [entries]; row_stride != 0: [nq][row_stride], entry j of query q's list at q * row_stride + j
  uint32_t row_stride;        // 0 = the ragged form
  uint32_t *pos_out;          // row_stride != 0: the scored position of every entry in the same layout, IDX_NONE for a skipped one
};

// halvings that take a run of qlen elements down to one: ceil(log2(qlen))
__device__ __forceinline__ uint32_t sparse_halvings(uint32_t qlen) { return qlen > 1 ? 32u - (uint32_t)__builtin_clz(qlen - 1) : 0u; }

// Stored elements [p, min(re, p + 64 U)) against the run in LDS, lane = element: acc plus this lane's products.  If the lane's
// index t is in the run at j, j stays inside [base, base + n) through every halving.
// L2: acc plus this lane's squares ((b - q)^2 on a hit, b^2 otherwise; qlen == 0 is served: no LDS read, every element adds b^2),
// mq plus the q^2 of its hits, hits plus their number.  Not L2: qlen > 0, and mq and hits are left alone.
template <int U, typename VT, bool L2>
__device__ __forceinline__ float sparse_lane_dot(const uint32_t *idx, const VT *val, uint64_t p, uint64_t re, const uint32_t *qi,
                                                 const VT *qv, uint32_t qlen, uint32_t steps, int lane, float acc, float &mq,
                                                 uint32_t &hits) {
  uint32_t t[U], base[U], n[U];
  float v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t e = p + (uint64_t)u * 64 + (uint32_t)lane;
    const bool in = e < re;
    t[u] = in ? idx[e] : 0u;
    v[u] = in ? (float)val[e] : 0.f;      // (a lane beyond the row holds 0)
    n[u] = in ? qlen : 0u;
    base[u] = 0;
  }
  for (uint32_t s = 0; s < steps; ++s) sparse_halve<U>(qi, t, base, n);
#pragma unroll
  for (int u = 0; u < U; ++u) sparse_match_step<VT, L2>(qi, qv, base[u], n[u], t[u], v[u], acc, mq, hits);
  return acc;
}

// L2: Qn of the run in LDS, the sum of its squares, the same bits in every lane (lane-strided fmaf, then the butterfly)
template <typename VT>
__device__ __forceinline__ float sparse_wave_run_norm(const VT *qv, uint32_t qlen, int lane) {
  float qn = 0.f;
  for (uint32_t i = lane; i < qlen; i += 64) {
    const float x = (float)qv[i];
    qn = __builtin_fmaf(x, x, qn);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
  return qn;
}

// The whole wave scores ONE stored row [rb, re) (wave-uniform) against the run in LDS, the same bits in every lane (lane-wise sums
// first, then the butterfly, whose order is fixed).  Not L2: minus the sum of value products over shared indices; a run of length
// 0 makes no LDS read and no load and scores 0.f - 0.f = +0.  L2: A + R; the butterfly adds up A, Mq and the hits, qn is the run's
// sparse_wave_run_norm.  No shortcut for a run of length 0 (the row's squares are summed) nor for an empty row (it scores R).
// (the inner step of sparse_rows_kernel and sparse_rows_dump_kernel; a narrow zvec_hip_sparse_search batch can walk its chunk of
// rows with it as well.)
template <typename VT, bool L2>
__device__ __forceinline__ float sparse_wave_row_score(const uint32_t *idx, const VT *val, uint64_t rb, uint64_t re, const uint32_t *qi,
                                                       const VT *qv, uint32_t qlen, uint32_t steps, int lane, float qn) {
  float acc = 0.f, mq = 0.f;
  uint32_t hits = 0;
  if (L2 || qlen != 0) {                // (uniform)
    uint64_t p = rb;
    for (; p < re && re - p > 64; p += 256) acc = sparse_lane_dot<4, VT, L2>(idx, val, p, re, qi, qv, qlen, steps, lane, acc, mq, hits);
    if (p < re) acc = sparse_lane_dot<1, VT, L2>(idx, val, p, re, qi, qv, qlen, steps, lane, acc, mq, hits);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if constexpr (L2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mq += __shfl_xor(mq, o);
        hits += __shfl_xor(hits, o);
      }
    }
  }
  return sparse_score<L2>(acc, mq, hits, qlen, qn);
}

// ONE query's run in LDS (indices | values, sparse_run_lds_bytes of it), the same in every lane of the wave that staged it
template <typename VT>
struct SparseRun {
  uint32_t *qi;               // [qlen] the query's indices
  VT *qv;                     // [qlen] its values, as stored
  uint32_t qlen;
  uint32_t steps;             // sparse_halvings(qlen)
  float qn;                   // L2: Qn, the sum of the run's squares (sparse_wave_run_norm); else 0
};

// The whole wave copies query q's run to LDS, once per work item.
template <typename VT, bool L2>
__device__ __forceinline__ SparseRun<VT> sparse_stage_run(const SparseOperands &o, uint32_t q, int lane) {
  extern __shared__ f32x4 zvk_smem4[];
  const uint32_t qb = o.q_off[q], qlen = min(o.q_off[q + 1] - qb, SPARSE_MAX_COUNT);
  uint32_t *qi = reinterpret_cast<uint32_t *>(zvk_smem4);
  VT *qv = reinterpret_cast<VT *>(qi + qlen);
  const VT *q_val = static_cast<const VT *>(o.q_val);
  for (uint32_t i = lane; i < qlen; i += 64) {
    qi[i] = o.q_idx[qb + i];
    qv[i] = q_val[qb + i];
  }
  const uint32_t steps = sparse_halvings(qlen);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  float qn = 0.f;
  if constexpr (L2) qn = sparse_wave_run_norm(qv, qlen, lane);
  return {qi, qv, qlen, steps, qn};
}

// Up to 64 rows, lane l holding the offsets [rb, re) of its own: the wave scores the rows of the lanes in `todo` one after the
// other (wave-uniform; the offsets are broadcast).  Returns this lane's own row's score, `out` for a lane that is not in `todo`.
template <typename VT, bool L2>
__device__ __forceinline__ float sparse_wave_score_rows(const SparseOperands &o, uint64_t todo, uint64_t rb, uint64_t re,
                                                        const uint32_t *qi, const VT *qv, uint32_t qlen, uint32_t steps, int lane,
                                                        float qn, float out) {
  while (todo) {                        // (uniform)
    const int j = __builtin_ctzll(todo);
    todo &= todo - 1;
    const float sc = sparse_wave_row_score<VT, L2>(o.idx, static_cast<const VT *>(o.val), bcast_u64(rb, j), bcast_u64(re, j), qi, qv,
                                                   qlen, steps, lane, qn);
    if (lane == j) out = sc;
  }
  return out;
}

template <typename VT, bool EXCL, bool L2 = false>
__global__ void __launch_bounds__(64) sparse_rows_kernel(const SparseRowsArgs a) {
  const int lane = threadIdx.x;
  const SparseOperands &o = a.op;
  const uint32_t q = a.item_q[blockIdx.x], e0 = a.item_e0[blockIdx.x];
  const uint32_t e1 = min(e0 + min(a.slice, SPARSE_ROWS_SLICE), a.list_off[q + 1]);
  const auto [qi, qv, qlen, steps, qn] = sparse_stage_run<VT, L2>(o, q, lane);

  // lane = listed entry: which entries are scored at all, and where their rows lie
  const uint32_t e = e0 + (uint32_t)lane;
  bool live = false;
  uint64_t rb = 0, re = 0;
  if (e < e1) {
    const uint32_t p = a.ids[e];
    live = p < a.n;
    if (EXCL) {
      if (live) live = ((o.exclude[p >> 5] >> (p & 31)) & 1u) == 0;
    }
    if (live) {
      rb = o.row_off[p];
      re = o.row_off[(uint64_t)p + 1];
    }
  }
  float out = __builtin_inff();
  out = sparse_wave_score_rows<VT, L2>(o, __ballot(live), rb, re, qi, qv, qlen, steps, lane, qn, out);
  if (e < e1) {
    if (a.row_stride == 0) {
      a.scores[e] = out;
    } else {          // (uniform) the grouped search's candidate matrix: the caller has filled the padding
      const size_t c = (size_t)q * a.row_stride + (e - a.list_off[q]);
      a.scores[c] = out;
      a.pos_out[c] = live ? a.ids[e] : IDX_NONE;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Score dump of a NARROW batch (the grouped full scan, FlatSparseEntity::search_group, flat_sparse_entity.h:79-103, which zvec calls
// one query at a time): sparse_scan_kernel is lane = query, so a batch of one leaves 63 of its 64 lanes idle.  Here the whole wave
// works on ONE stored row (sparse_wave_row_score, lane = stored element).  One wave per work-group; a work item is (query, chunk of
// rows), the chunk a multiple of 64 rows.  The query's run is copied to LDS once per item (32 KiB at most).  The wave takes 64 rows
// at a time: lane l looks at row base + l — excluded (nothing of it is fetched) or its two offsets, one coalesced load each — then
// the rows that hold anything are scored one after the other (wave-uniform; the offsets are broadcast), lane l keeps row base + l's
// score, and ONE coalesced store writes the 64 scores to dump[(q - qsub0) * n + base ..]: +inf for an excluded row, exactly +0 for
// a row or a query without elements (a run of length 0 reads no row at all).  L2: an empty row scores Qn, and a run of length 0
// skips nothing (every row that holds anything is read and scores the sum of its squares).
struct SparseRowsDumpArgs {
  SparseOperands op;
  uint32_t qsub0;             // the query whose scores are row 0 of `dump`
  uint32_t nqsub;             // queries of this launch: qsub0 .. qsub0 + nqsub
  uint64_t n;                 // rows
  uint32_t rows_per_chunk;    // a multiple of 64
  float *dump;                // [nqsub][n]
};

template <typename VT, bool EXCL, bool L2 = false>
__global__ void __launch_bounds__(64) sparse_rows_dump_kernel(const SparseRowsDumpArgs a) {
  const int lane = threadIdx.x;
  const SparseOperands &o = a.op;
  // (the queries of one chunk are neighbours in the grid: they read the same rows)
  const uint32_t chunk = blockIdx.x / a.nqsub, qs = blockIdx.x - chunk * a.nqsub, q = a.qsub0 + qs;
  const auto [qi, qv, qlen, steps, qn] = sparse_stage_run<VT, L2>(o, q, lane);

  float *out = a.dump + (size_t)qs * a.n;
  const uint64_t r0 = (uint64_t)chunk * a.rows_per_chunk, r1 = min(a.n, r0 + a.rows_per_chunk);
  for (uint64_t base = r0; base < r1; base += 64) {
    const uint64_t r = base + (uint32_t)lane;
    bool live = r < r1;
    if (EXCL) {
      if (live) live = ((o.exclude[r >> 5] >> (r & 31)) & 1u) == 0;
    }
    float s = live ? (L2 ? qn : 0.f) : __builtin_inff();      // (L2: an empty row scores R = Qn, +0 for a run of length 0)
    if (L2 || qlen != 0) {              // (uniform)
      uint64_t rb = 0, re = 0;
      if (live) {
        rb = o.row_off[r];
        re = o.row_off[r + 1];
      }
      s = sparse_wave_score_rows<VT, L2>(o, __ballot(re > rb), rb, re, qi, qv, qlen, steps, lane, qn, s);
    }
    if (r < r1) out[r] = s;
  }
}

// Query staging.  A block's runs are contiguous in the CSR query arrays, so those arrays ARE the LDS images, block after block (the
// scan copies [q_off[first], q_off[last + 1]) verbatim); the offsets and the block table are one small host-made plan.  What is left
// to stage per search are the shared bounds: they start at +inf (the threshold is a separate, non-strict test).
__global__ void __launch_bounds__(256) sparse_prep_queries_kernel(uint32_t nq, uint32_t *gtau) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nq) gtau[i] = fkey(__builtin_inff());
}

// get_vector: row `pos` -> out[0] = count, out[4 .. 4 + count) indices, then the values as stored, back to back (VT each)
template <typename VT>
__global__ void __launch_bounds__(256) sparse_unpack_kernel(const uint64_t *row_off, const uint32_t *idx, const VT *val, uint64_t pos,
                                                            uint32_t *out) {
  const uint64_t b = row_off[pos];
  const uint32_t c = (uint32_t)min((uint64_t)SPARSE_MAX_COUNT, row_off[pos + 1] - b);
  if (threadIdx.x == 0) out[0] = c;
  for (uint32_t i = threadIdx.x; i < c; i += 256) {
    out[4 + i] = idx[b + i];
    if constexpr (sizeof(VT) == 4) out[4 + SPARSE_MAX_COUNT + i] = __builtin_bit_cast(uint32_t, val[b + i]);
    else reinterpret_cast<VT *>(out + 4 + SPARSE_MAX_COUNT)[i] = val[b + i];
  }
}

}  // namespace zvk
