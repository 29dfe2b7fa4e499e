// zvk_hnsw_sparse.hip.h — SPARSE rows in the HNSW kernels (zvec_hip_hnsw_sparse_*, api_entry_hnsw_sparse.inc.h and
// api_entry_hnsw_sparse_build.inc.h): the scorer; the search kernel, which is the walk of zvk_hnsw.hip.h (hnsw_greedy, hnsw_beam,
// hnsw_emit, none of it copied) behind a query staged as a run; and HnswCsrRows<VT>, the model that the build kernels of
// zvk_hnsw_build.hip.h are instantiated for.  Reference: src/core/algorithm/hnsw_sparse/hnsw_sparse_algorithm.cc,
// which is hnsw_algorithm.cc line for line but for dc.dist(...) on a sparse row; under InnerProductSparse that is
// MinusInnerProductSparseMatrix<T>::Compute (src/ailego/math/inner_product_matrix.h:2781-2862): minus the sum of value products over
// shared indices, exactly +0.0 when no index is shared.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Rows are CSR as in the sparse flat store (zvk_sparse.hip.h): row_off[n + 1] (u64), idx (u32, strictly ascending inside a row), val
// (VT: float or _Float16).  The query's run lies in LDS as sparse_stage_run leaves it: indices, then values as stored.  Halves are
// widened where they are read; every product is one fp32 fmaf; no half arithmetic.
//
// Scorer (HnswSparseScorer).  The walk hands over up to 64 collected nodes.  Lane r < nc fetches the two offsets of row coll[r] into
// LDS.  Then SIXTEEN lanes take a row and four rows are in flight per wave: lane `sub` of a group owns the stored elements
// sub, sub + 16, sub + 32, ... of its row and takes TWO of them per step (sub + 32 j and sub + 32 j + 16), each lower-bounded in the
// query's run by the wave-uniform number of halvings of the run's length (sparse_halve<2>: two independent chains of dependent LDS
// reads), then one equality probe and, on a hit, one fmaf (sparse_match_step<VT, false>).  The first step's index and value loads
// of the next four rows are requested before the current four are reduced.
//
// Summation order, a function of the (row, query) pair alone.  Element e of the row belongs to lane e % 16 of whichever group took
// the row; that lane adds the products of its elements to one fp32 accumulator in ascending e, one fmaf per matched element,
// starting from +0; the sixteen accumulators are then added by the fixed butterfly __shfl_xor 8, 4, 2, 1 inside the group, and the
// score is 0.f - sum.  Neither the group, the slot in `coll`, nor the other rows of the batch enter.  A query run of length 0 reads
// neither LDS nor a row and scores every node 0.f - 0.f = +0; an empty row reads nothing either and scores +0.
//
// Roles in the build.  The scorer wants one operand staged in LDS and streams the other from CSR.  Slot 0 holds the BASE of the
// wave's work: the new node's row in the insert kernel, the target's row in a reverse group.  Slot 1 holds the keep rule's current
// candidate c.  A score's bits depend on the (staged run, streamed row) pair alone, as in the search.  d(c, s) of the keep rule is
// (c staged, s streamed); it is compared with d(c, base), which came out of the walk or the sort as (base staged, c streamed).  On
// real values the two roles may differ in the last bit; integer-valued data is exact either way.
#pragma once
#include "zvk_hnsw.hip.h"
#include "zvk_sparse.hip.h"

namespace zvk {

struct HnswSparseArgs {
  HnswArgs g;                 // the graph, the walk's parameters, workspace and outputs; rows, dim, dpad, ip and queries are not read
  SparseOperands op;          // the stored rows and the WHOLE batch's queries (q_off [count + 1]); exclude is g.exclude's
  uint32_t q0;                // the batch query that work-group 0 of this launch walks for
  uint32_t run_bytes;         // LDS set aside for the run: hnsw_sparse_run_bytes of the batch's longest
};

// a run's slot in LDS, the next slot or the words of R behind it 8-byte aligned
__host__ __device__ inline size_t hnsw_sparse_run_bytes(uint32_t run_elems, uint32_t width) {
  return (sparse_run_lds_bytes(run_elems, width) + 7) & ~(size_t)7;
}

template <typename VT>
struct HnswSparseScorer {
  const uint64_t *row_off;
  const uint32_t *idx;
  const VT *val;
  const uint32_t *qi;         // the run in LDS
  const VT *qv;
  uint32_t qlen, steps;       // wave-uniform
  uint64_t *rbeg;             // [64] LDS: where the collected rows begin
  uint32_t *rlen;             // [64] LDS: their lengths

  // cdist[r] = the score of row coll[r] for r < nc (nc <= 64)
  __device__ __forceinline__ void operator()(const HnswArgs &, const uint32_t *coll, float *cdist, uint32_t nc, int lane) const {
    if (qlen == 0) {                                     // (uniform) nothing is shared with an empty run
      if ((uint32_t)lane < nc) cdist[lane] = 0.f - 0.f;
      hnsw_sync(false);
      return;
    }
    const uint32_t grp = (uint32_t)lane >> 4, sub = (uint32_t)lane & 15u;
    if ((uint32_t)lane < nc) {
      const uint32_t node = coll[lane];
      const uint64_t b = row_off[node];
      rbeg[lane] = b;
      rlen[lane] = (uint32_t)min((uint64_t)SPARSE_MAX_COUNT, row_off[(size_t)node + 1] - b);
    }
    hnsw_sync(false);
    uint32_t r = grp, len = r < nc ? rlen[r] : 0u;
    uint64_t b = r < nc ? rbeg[r] : 0ull;
    uint32_t t[2] = {0u, 0u};
    float v[2] = {0.f, 0.f};
    if (sub < len) { t[0] = idx[b + sub]; v[0] = (float)val[b + sub]; }
    if (sub + 16 < len) { t[1] = idx[b + sub + 16]; v[1] = (float)val[b + sub + 16]; }
    for (uint32_t g = 0; g < nc; g += 4) {
      float acc = 0.f, mq = 0.f;                         // (mq and hits are the L2 form's: left alone here)
      uint32_t hits = 0;
      for (uint32_t e = sub; e < len;) {                 // (groups differ in length: the wave runs the longest row's steps)
        uint32_t base[2] = {0u, 0u}, n[2] = {qlen, e + 16 < len ? qlen : 0u};
        for (uint32_t s = 0; s < steps; ++s) sparse_halve<2>(qi, t, base, n);
        sparse_match_step<VT, false>(qi, qv, base[0], n[0], t[0], v[0], acc, mq, hits);
        sparse_match_step<VT, false>(qi, qv, base[1], n[1], t[1], v[1], acc, mq, hits);
        e += 32;
        if (e < len) { t[0] = idx[b + e]; v[0] = (float)val[b + e]; }
        if (e + 16 < len) { t[1] = idx[b + e + 16]; v[1] = (float)val[b + e + 16]; }
      }
      const uint32_t rcur = r;
      r += 4;
      if (g + 4 < nc) {                                  // the next rows' first loads go out before the reduction below
        len = r < nc ? rlen[r] : 0u;
        b = r < nc ? rbeg[r] : 0ull;
        if (sub < len) { t[0] = idx[b + sub]; v[0] = (float)val[b + sub]; }
        if (sub + 16 < len) { t[1] = idx[b + sub + 16]; v[1] = (float)val[b + sub + 16]; }
      }
      acc += __shfl_xor(acc, 8, 16);
      acc += __shfl_xor(acc, 4, 16);
      acc += __shfl_xor(acc, 2, 16);
      acc += __shfl_xor(acc, 1, 16);
      if (sub == 0 && rcur < nc) cdist[rcur] = 0.f - acc;
    }
    hnsw_sync(false);
  }
};

// The model of CSR rows for the build kernels (zvk_hnsw.hip.h, "The model of a row kind"); of the HnswArgs beside it rows, dim, dpad,
// ip and queries are not read.  A slot is a run as sparse_stage_run lays it out: indices, then values as stored.
template <typename VT>
struct HnswCsrRows {
  typedef HnswSparseScorer<VT> Scorer;
  static constexpr uint32_t SCRATCH = 64 * 8 + 64 * 4;      // the begins (u64) and the lengths of the collected rows
  SparseOperands op;          // the stored rows
  uint32_t run_elems;         // what a slot has room for: the longest row of the build

  __host__ __device__ __forceinline__ size_t slot_bytes(const HnswArgs &) const { return hnsw_sparse_run_bytes(run_elems, sizeof(VT)); }

  // (rows are read with u64 offsets; sparse_stage_run reads query arrays with u32 offsets)
  __device__ __forceinline__ Scorer stage_row(const HnswArgs &, unsigned char *slot, unsigned char *scratch, uint32_t node, int lane) const {
    const VT *val = static_cast<const VT *>(op.val);
    const uint64_t rb = hnsw_uni64(op.row_off[node]);
    const uint32_t len = (uint32_t)min((uint64_t)run_elems, hnsw_uni64(op.row_off[(size_t)node + 1]) - rb);
    uint32_t *qi = reinterpret_cast<uint32_t *>(slot);
    VT *qv = reinterpret_cast<VT *>(qi + len);
    for (uint32_t e = (uint32_t)lane; e < len; e += 64) {
      qi[e] = op.idx[rb + e];
      qv[e] = val[rb + e];
    }
    hnsw_sync(false);
    uint64_t *rbeg = reinterpret_cast<uint64_t *>(scratch);
    return Scorer{op.row_off, op.idx, val, qi, qv, len, sparse_halvings(len), rbeg, reinterpret_cast<uint32_t *>(rbeg + 64)};
  }
};

// One wave per query, one wave per work-group, as hnsw_search_kernel, whose steps these are; a kernel of its own because the folded
// one is slower on the dense kinds.  run | R [ef] | C [HNSW_C_LDS] | row begins [64] (u64) | coll [64] | cdist [64] |
// row lengths [64]: hnsw_walk_lds_bytes of one slot of s.run_bytes and HnswCsrRows<VT>::SCRATCH.
template <typename VT>
__global__ __launch_bounds__(64) void hnsw_sparse_search_kernel(HnswSparseArgs s) {
  extern __shared__ f32x4 zvk_smem4[];
  const HnswArgs &a = s.g;
  const int lane = (int)threadIdx.x;
  const uint32_t q = blockIdx.x;
  const SparseRun<VT> run = sparse_stage_run<VT, false>(s.op, s.q0 + q, lane);
  uint64_t *R = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(zvk_smem4) + s.run_bytes);
  uint64_t *C = R + a.ef;
  uint64_t *rbeg = C + HNSW_C_LDS;
  uint32_t *coll = reinterpret_cast<uint32_t *>(rbeg + 64);
  float *cdist = reinterpret_cast<float *>(coll + 64);
  uint32_t *rlen = reinterpret_cast<uint32_t *>(cdist + 64);
  const HnswSparseScorer<VT> score{s.op.row_off, s.op.idx, static_cast<const VT *>(s.op.val), run.qi, run.qv, run.qlen, run.steps, rbeg, rlen};
  if (lane == 0) coll[0] = a.entry;
  hnsw_sync(false);

  // the four steps of the rule, as hnsw_search_kernel takes them
  uint32_t scanned = 1, hops = 0, ep = a.entry;
  score(a, coll, cdist, 1, lane);
  float dist = cdist[0];
  hnsw_sync(false);
  for (uint32_t l = a.max_level; l >= 1; --l) hnsw_greedy(a, l, score, coll, cdist, ep, dist, scanned, lane);
  const uint32_t rsize = hnsw_beam(a, 0, score, R, C, a.cand_ws != nullptr ? a.cand_ws + (size_t)q * a.ccap : nullptr, coll, cdist,
                                   a.visited + (size_t)q * a.vis_words, ep, dist, scanned, hops, lane);
  hnsw_emit(a, q, R, rsize, scanned, hops, lane);
}

}  // namespace zvk
