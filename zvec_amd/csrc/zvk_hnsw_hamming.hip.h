// zvk_hnsw_hamming.hip.h — the distance step of the HNSW walk over binary rows under the Hamming distance (zvec_hip_hnsw_create_binary,
// api_entry_hnsw.inc.h): score = (float) popcount(row ^ query), an exact integer.  The walk, the build and the group-by stages are
// those of zvk_hnsw.hip.h, zvk_hnsw_build.hip.h and zvk_hnsw_group.hip.h, instantiated for HnswRows<HNSW_BITS>; this file is the scorer
// they take and HnswDenseKind<HNSW_BITS>, which tells that model that a row in LDS is words, copied as they are.  DESIGN §3c "Binary rows".
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Stored rows are [n][wpad] uint32_t words, words = bits / 32 rounded up to 4 and zero padded, so every row is 16-byte aligned and a
// lane loads one 16-byte chunk per step (BINARY64 rows are the same bytes: the host is little-endian).  The query, or the
// build's candidate or base row, is wpad words in LDS, read 16 bytes at a time; the lanes of different rows that hold the same
// chunk number read one address, which LDS broadcasts.
//
// The lane split is not the dense one (sixteen lanes a row whatever the dimension): a bit row is 32 times shorter than the fp32 row
// of the same dimension and most are a handful of chunks, so G lanes take a row, G the smallest power of two >= chunks, at most 16,
// and 64 / G rows are in flight per wave.  A 128-bit row is one lane's one load, no cross-lane step at all, and a 64-entry
// neighbour list is scored in one pass; a row of 2048 bits or more takes sixteen lanes that stride by sixteen chunks.
#pragma once
#include "zvk_hnsw.hip.h"

namespace zvk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the lanes that take one row of `wpad` words, as log2: 0 .. 4
__host__ __device__ inline uint32_t hnsw_hamming_lanes_log2(uint32_t wpad) {
  const uint32_t chunks = wpad >> 2;
  uint32_t lg = 0;
  while (lg < 4 && (1u << lg) < chunks) ++lg;
  return lg;
}

// The per-chunk step of the Hamming distance (the Acc of hnsw_chunk_distances below): acc + popcount(b ^ x), scored as it stands
struct HnswPopcAcc {
  __device__ __forceinline__ uint32_t add(u32x4 b, u32x4 x, uint32_t acc) const {
    acc += (uint32_t)__builtin_popcount(b.x ^ x.x);        // (v_bcnt_u32_b32 adds its second operand)
    acc += (uint32_t)__builtin_popcount(b.y ^ x.y);
    acc += (uint32_t)__builtin_popcount(b.z ^ x.z);
    acc += (uint32_t)__builtin_popcount(b.w ^ x.w);
    return acc;
  }
  __device__ __forceinline__ float score(uint32_t acc) const { return (float)acc; }
};

// cdist[r] = f.score(the sum over the 16-byte chunks of f.add(chunk of row coll[r], chunk of the wpad words at qw in LDS)) for
// r < nc (nc <= 64): the loop of every kind whose rows are words and whose score is an integer sum (bits here, int8 values in
// zvk_hnsw_i8.hip.h).  G lanes take a row, one chunk each per step, 64 / G rows in flight; the first chunk of the next 64 / G rows
// is requested before the current ones are reduced across their G lanes.  Rows r >= nc of the last batch load row coll[0] and write
// nothing.  Integer sums modulo 2^32: no order to pin.
template <uint32_t G, typename Acc>
__device__ __forceinline__ void hnsw_chunk_distances(const HnswArgs &a, const uint32_t *qw, const uint32_t *coll, float *cdist, uint32_t nc,
                                                     int lane, Acc f) {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "a row is taken by a power of two of lanes, at most 16");
  constexpr uint32_t ROWS = 64 / G;
  const uint32_t grp = (uint32_t)lane / G, sub = (uint32_t)lane % G;
  const uint32_t nv = a.dpad >> 2;                         // chunks of a row: nv <= G unless G == 16
  const u32x4 *q4 = reinterpret_cast<const u32x4 *>(qw);
  const u32x4 *rows4 = static_cast<const u32x4 *>(a.rows);
  const u32x4 zero = {0u, 0u, 0u, 0u};
  uint32_t r = grp;
  const u32x4 *row = rows4 + (size_t)coll[r < nc ? r : 0] * nv;
  u32x4 b0 = sub < nv ? row[sub] : zero;
  for (uint32_t g = 0; g < nc; g += ROWS) {
    uint32_t acc = 0;
    if (sub < nv) acc = f.add(b0, q4[sub], 0u);
    if constexpr (G == 16) {
#pragma unroll 4
      for (uint32_t t = sub + 16; t < nv; t += 16) acc = f.add(row[t], q4[t], acc);
    }
    const uint32_t rcur = r;
    r += ROWS;
    row = rows4 + (size_t)coll[r < nc ? r : 0] * nv;
    if (g + ROWS < nc) b0 = sub < nv ? row[sub] : zero;    // the next rows' first loads go out before the reduction below
#pragma unroll
    for (uint32_t o = G >> 1; o >= 1; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, (int)o, (int)G);
    if (sub == 0 && rcur < nc) cdist[rcur] = f.score(acc);
  }
  hnsw_sync(false);
}

// the lane split of a handle's row width, uniform over the wave and over the launch: G depends on a.dpad alone
template <typename Acc>
__device__ __forceinline__ void hnsw_chunk_distances_any(const HnswArgs &a, const uint32_t *qw, const uint32_t *coll, float *cdist, uint32_t nc,
                                                         int lane, Acc f) {
  switch (hnsw_hamming_lanes_log2(a.dpad)) {
    case 0: hnsw_chunk_distances<1>(a, qw, coll, cdist, nc, lane, f); break;
    case 1: hnsw_chunk_distances<2>(a, qw, coll, cdist, nc, lane, f); break;
    case 2: hnsw_chunk_distances<4>(a, qw, coll, cdist, nc, lane, f); break;
    case 3: hnsw_chunk_distances<8>(a, qw, coll, cdist, nc, lane, f); break;
    default: hnsw_chunk_distances<16>(a, qw, coll, cdist, nc, lane, f); break;
  }
}

// The scorer of the walk over binary rows (the contract of HnswDenseScorer, zvk_hnsw.hip.h) against the words at qw in LDS.
struct HnswHammingScorer {
  const uint32_t *qw;
  __device__ __forceinline__ void operator()(const HnswArgs &a, const uint32_t *coll, float *cdist, uint32_t nc, int lane) const {
    hnsw_chunk_distances_any(a, qw, coll, cdist, nc, lane, HnswPopcAcc());
  }
};

template <>
struct HnswDenseKind<HNSW_BITS> {
  typedef uint32_t lds;
  typedef HnswHammingScorer Scorer;
  static __device__ __forceinline__ uint32_t word(const void *p, size_t i) { return static_cast<const uint32_t *>(p)[i]; }
};

}  // namespace zvk
