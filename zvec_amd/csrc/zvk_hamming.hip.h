// zvk_hamming.hip.h — binary rows under the Hamming metric: blocked layout, pack / unpack, the XOR + population-count scan, the
// fp32 -> sign-bit encoder.
// Part of the device code of libzvec_hip (included through scan_kernels.hip.h).
//
// Reference: HammingMetric (src/core/metric/hamming_metric.cc) over HammingDistanceMatrix<uint32_t / uint64_t, 1, 1>
// (src/ailego/math/hamming_distance_matrix.h): score = (float) popcount(row ^ query), smaller is better.
//
// Layout.  A row of `dim` bits is `dim / 32` words, stored as ceil(words / 4) 16-byte chunks (zero padded).  The 128-row tile
// of the fp stores is kept (positions, holes, exclude bits and the key column are the same arithmetic); inside a tile the data
// is ordered [chunk][row], so a wave in which lane = row reads 64 x 16 B = 1 KiB contiguous per chunk.  No norm column.
//
// Scan.  The transpose of the MFMA scans: ONE wave per work-group owns both halves of a tile (rows `lane` and `lane + 64`, their
// words in VGPRs) and loops over the up to 32 queries of its query block; the query words are wave-uniform and come through the
// scalar data cache, so a 32-bit word of a (row, query) pair costs one v_xor_b32 and one accumulating v_bcnt_u32_b32 and nothing
// else.  The 32 x 2 distances of a tile stay in VGPRs until the tile is done; then every query's two rows of scores meet that
// query's bound.  Admission is STRICT once a list is full (Hamming scores tie massively; a tie at the k-th place is never needed)
// and also strict against the bound the work-groups of the same query share (`gtau`, a full list's k-th score somewhere).
#pragma once
#include "zvk_common.hip.h"

namespace zvk {

constexpr int HAM_QB = 32;            // queries per query block (one accumulator pair per query and lane)
constexpr uint32_t HAM_FUSED_MAX_K = 128;   // longer lists take the dense-score route (host: flat_scan_hamming)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// query words are read through the constant address space: a uniform address there is a scalar load (SGPR operands for the
// v_xor), whatever the kernel stores elsewhere.  The prepared queries are written by an earlier launch and never by the scan.
typedef const __attribute__((address_space(4))) u32x4 *ham_qptr;

// word offset of 16-byte chunk `c` of the row at padded position `pos` (cpr = chunks per row)
__host__ __device__ inline size_t ham_offset(uint64_t pos, uint32_t c, uint32_t cpr) {
  return ((size_t)(pos >> 7) * cpr + c) * (TILE_N * 4) + (size_t)(pos & 127) * 4;
}

struct HamScanArgs {
  const uint32_t *base;       // blocked binary rows
  const uint32_t *exclude;    // nullable bitset over positions (holes included), set = skip
  const uint32_t *queries;    // [nq][cpr * 4] words, zero padded
  uint32_t cpr;               // 16-byte chunks per row
  uint32_t k;
  float threshold;
  uint32_t nq;
  uint64_t n;                 // positions in use
  uint32_t ntiles;
  uint32_t tiles_per_chunk;
  uint32_t nchunks;
  uint32_t nqblocks;
  uint32_t *gtau;             // [nq] shared bounds (fkey of a full list's k-th score; +inf at the start)
  float *dump;                // DUMP: [nq][dump_stride] scores, +inf for padding / excluded positions
  uint32_t dump_stride;
  float *part_s;              // [nq][nchunks][k]
  uint32_t *part_i;
};

__host__ __device__ inline size_t ham_lds_bytes(uint32_t k) { return ((size_t)HAM_QB * 3 + 2 * (size_t)HAM_QB * k) * 4; }

// CH chunks of both rows of the lane against every query of the block.  The words of query j + 1 are fetched (scalar loads) in
// front of the popcounts of query j; the uniform guards keep the fetches of the queries after that from being scheduled early too,
// which would take 16 SGPRs per query.
// INDIRECT (the list scan, zvk_hamming_ivf.hip.h): query j of the block does not start at chunk j * qstride of `q` but at the chunk
// lane j of `qv` names — a v_readlane away from a scalar, so nothing else changes.
template <int CH, bool INDIRECT = false>
__device__ __forceinline__ void ham_accumulate(const uint32_t *tile, ham_qptr q, uint32_t qstride, uint32_t c0, uint32_t nqb, int lane,
                                               uint32_t (&acc)[HAM_QB][2], uint32_t qv = 0) {
  // (the query words do not depend on the tile: without this the compiler hoists the loads of the last chunks of all 32 queries
  // out of the tile loop, into SGPRs that do not exist)
  asm volatile("" : "+s"(c0), "+s"(nqb));        // (nqb: the 32 guards below are compared where they branch, not kept in 64 SGPRs)
  u32x4 r0[CH], r1[CH], cur[CH], nxt[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const uint32_t *p = tile + (size_t)(c0 + c) * (TILE_N * 4) + lane * 4;
    r0[c] = *reinterpret_cast<const u32x4 *>(p);
    r1[c] = *reinterpret_cast<const u32x4 *>(p + 64 * 4);
    if constexpr (INDIRECT) cur[c] = q[bcast_u(qv, 0) + c0 + c];
    else cur[c] = q[c0 + c];
  }
#pragma unroll
  for (int j = 0; j < HAM_QB; ++j) {
    if ((uint32_t)j < nqb) {                       // (uniform)
      const uint32_t jn = min((uint32_t)j + 1, nqb - 1);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if constexpr (INDIRECT) nxt[c] = q[bcast_u(qv, (int)jn) + c0 + c];
        else nxt[c] = q[(size_t)jn * qstride + c0 + c];
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[j][0] = __builtin_popcount(r0[c][e] ^ cur[c][e]) + acc[j][0];
          acc[j][1] = __builtin_popcount(r1[c][e] ^ cur[c][e]) + acc[j][1];
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) cur[c] = nxt[c];
    }
  }
}

// One wave per work-group; item = (chunk of tiles, query block).  DUMP: every score goes to the [query][position] matrix and
// nothing is selected (large k, selected by merge_kernel).
template <bool EXCL, bool DUMP>
__global__ void __launch_bounds__(64) hamming_scan_kernel(const HamScanArgs a) {
  extern __shared__ f32x4 zvk_smem4[];
  float *tau = reinterpret_cast<float *>(zvk_smem4);                // [QB] k-th score of a full list, +inf before
  uint32_t *cnt = reinterpret_cast<uint32_t *>(tau + HAM_QB);       // [QB]
  float *gt = reinterpret_cast<float *>(cnt + HAM_QB);              // [QB] shared bound as of this tile
  float *Ls = gt + HAM_QB;                                          // [QB][k]
  uint32_t *Li = reinterpret_cast<uint32_t *>(Ls + (size_t)HAM_QB * a.k);
  const int lane = threadIdx.x;
  const uint32_t chunk = blockIdx.x / a.nqblocks, qb = blockIdx.x - chunk * a.nqblocks;
  const uint32_t q0 = qb * HAM_QB, nqb = min((uint32_t)HAM_QB, a.nq - q0);
  const uint32_t k = a.k, cpr = a.cpr;
  const ham_qptr qp = (ham_qptr)(uintptr_t)(a.queries + (size_t)q0 * cpr * 4);
  if (!DUMP) {
    if (lane < HAM_QB) { tau[lane] = __builtin_inff(); cnt[lane] = 0; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  const uint32_t t0 = chunk * a.tiles_per_chunk, t1 = min(a.ntiles, t0 + a.tiles_per_chunk);
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t *tile = a.base + (size_t)t * cpr * (TILE_N * 4);
    // (per tile and opaque: the guards and per-query addresses below are recomputed where they are used instead of living in
    // a hundred SGPRs across the tile loop)
    uint32_t nqt = nqb, jz = 0;
    asm volatile("" : "+s"(nqt), "+s"(jz));
    uint32_t acc[HAM_QB][2];
#pragma unroll
    for (int j = 0; j < HAM_QB; ++j) { acc[j][0] = 0; acc[j][1] = 0; }
    uint32_t c = 0;
    for (; c + 4 <= cpr; c += 4) ham_accumulate<4>(tile, qp, cpr, c, nqb, lane, acc);
    if (c + 2 <= cpr) { ham_accumulate<2>(tile, qp, cpr, c, nqb, lane, acc); c += 2; }
    if (c < cpr) ham_accumulate<1>(tile, qp, cpr, c, nqb, lane, acc);
    const uint64_t p0 = (uint64_t)t * TILE_N + lane, p1 = p0 + 64;
    bool ok0 = p0 < a.n, ok1 = p1 < a.n;
    if (EXCL) {
      if (ok0) ok0 = ((a.exclude[p0 >> 5] >> (p0 & 31)) & 1u) == 0;
      if (ok1) ok1 = ((a.exclude[p1 >> 5] >> (p1 & 31)) & 1u) == 0;
    }
    if (DUMP) {
#pragma unroll
      for (int j = 0; j < HAM_QB; ++j) {
        if ((uint32_t)j < nqt) {
          float *row = a.dump + (size_t)(q0 + jz + j) * a.dump_stride;
          row[p0] = ok0 ? (float)acc[j][0] : __builtin_inff();
          row[p1] = ok1 ? (float)acc[j][1] : __builtin_inff();
        }
      }
      continue;
    }
    // the bounds the work-groups of these queries have published so far
    if ((uint32_t)lane < nqb) gt[lane] = fkey_inv(a.gtau[q0 + lane]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < HAM_QB; ++j) {
      if ((uint32_t)j < nqt) {
        const float s0 = ok0 ? (float)acc[j][0] : __builtin_inff(), s1 = ok1 ? (float)acc[j][1] : __builtin_inff();
        const float tg = gt[j];
        float tl = tau[j];
        float b = fminf(tl, tg);
        uint64_t m0 = __ballot(s0 <= a.threshold && s0 < b), m1 = __ballot(s1 <= a.threshold && s1 < b);
        if ((m0 | m1) == 0) continue;
        uint32_t n_in = cnt[j];
        float *L = Ls + (size_t)(jz + j) * k;
        uint32_t *I = Li + (size_t)(jz + j) * k;
        bool improved = false;
        while ((m0 | m1) != 0) {
          int l;
          float cs;
          uint32_t ci;
          if (m0 != 0) {
            l = __builtin_ctzll(m0);
            cs = bcast_f(s0, l);
            ci = t * TILE_N + (uint32_t)l;
            m0 &= m0 - 1;
          } else {
            l = __builtin_ctzll(m1);
            cs = bcast_f(s1, l);
            ci = t * TILE_N + 64u + (uint32_t)l;
            m1 &= m1 - 1;
          }
          // (sorted_insert sets tl to the k-th score once the list is full; until then it stays +inf)
          if (sorted_insert<false>(L, nullptr, I, k, n_in, cs, 0u, ci, lane, tl)) {
            if (n_in == k) {
              improved = true;
              b = fminf(tl, tg);
              m0 &= __ballot(s0 < b);
              m1 &= __ballot(s1 < b);
            }
          }
        }
        if (lane == 0) {
          cnt[j] = n_in;
          tau[j] = tl;
          if (improved && tl < tg) atomicMin(&a.gtau[q0 + j], fkey(tl));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (DUMP) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = 0; j < nqb; ++j) {
    const size_t slot = (size_t)(q0 + j) * a.nchunks + chunk;
    const uint32_t c = cnt[j];
    for (uint32_t e = lane; e < k; e += 64) {
      a.part_s[slot * k + e] = e < c ? Ls[(size_t)j * k + e] : __builtin_inff();
      a.part_i[slot * k + e] = e < c ? Li[(size_t)j * k + e] : IDX_NONE;
    }
  }
}

// scattered rows against their queries (search_by_ids, batch_distance): one thread per (query, list entry), the outputs of
// pkeys_score_kernel — out_s / out_i [nq][maxlen], holes and the unused tail +inf / IDX_NONE
__global__ void __launch_bounds__(256) hamming_pkeys_kernel(const uint32_t *base, const uint32_t *queries, uint32_t cpr, const uint32_t *pos,
                                                            const uint32_t *off, uint32_t nq, uint32_t maxlen, float *out_s, uint32_t *out_i) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (uint64_t)nq * maxlen) return;
  const uint32_t q = (uint32_t)(w / maxlen), j = (uint32_t)(w - (uint64_t)q * maxlen);
  const uint32_t len = off[q + 1] - off[q];
  const uint32_t id = j < len ? pos[off[q] + j] : IDX_NONE;
  float s = __builtin_inff();
  if (id != IDX_NONE) {
    uint32_t acc = 0;
    for (uint32_t c = 0; c < cpr; ++c) {
      const u32x4 r = *reinterpret_cast<const u32x4 *>(base + ham_offset(id, c, cpr));
      const u32x4 v = *reinterpret_cast<const u32x4 *>(queries + ((size_t)q * cpr + c) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_popcount(r[e] ^ v[e]) + acc;
    }
    s = (float)acc;
  }
  out_s[w] = s;
  out_i[w] = id;
}

// queries [nq][words] -> [nq][cpr * 4] zero padded; the shared bounds start at +inf (the threshold is a separate, non-strict test)
__global__ void __launch_bounds__(256) hamming_prep_queries_kernel(const uint32_t *src, uint32_t nq, uint32_t words, uint32_t cpr, uint32_t *dst,
                                                                   uint32_t *gtau) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t wpad = cpr * 4;
  if (i < nq) gtau[i] = fkey(__builtin_inff());
  if (i >= (uint64_t)nq * wpad) return;
  const uint32_t q = (uint32_t)(i / wpad), w = (uint32_t)(i - (uint64_t)q * wpad);
  dst[i] = w < words ? src[(size_t)q * words + w] : 0u;
}

// rows [n][words] (row-major) -> blocked positions pos0 + i (or dst_pos[i]), zero padded to whole chunks; keys as pack_rows_kernel
__global__ void __launch_bounds__(256) hamming_pack_kernel(const uint32_t *src, uint64_t n, uint32_t words, uint32_t cpr, const uint64_t *src_row,
                                                           uint64_t pos0, const uint64_t *dst_pos, uint32_t *base, uint64_t *keys_out,
                                                           const uint64_t *key_src) {
  const int lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const uint64_t sr = src_row ? src_row[i] : i, pos = dst_pos ? dst_pos[i] : pos0 + i;
  for (uint32_t w = lane; w < cpr * 4; w += 64) base[ham_offset(pos, w >> 2, cpr) + (w & 3)] = w < words ? src[(size_t)sr * words + w] : 0u;
  if (lane == 0 && keys_out) keys_out[pos] = key_src ? key_src[i] : pos;
}

// blocked rows -> plain rows for a list of positions (pos == nullptr: the one position pos1); one work-group per position
__global__ void __launch_bounds__(256) hamming_unpack_kernel(const uint32_t *base, const uint64_t *pos, uint64_t pos1, uint32_t words, uint32_t cpr,
                                                             uint32_t *out) {
  const uint64_t p = pos ? pos[blockIdx.x] : pos1;
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) out[(size_t)blockIdx.x * words + w] = base[ham_offset(p, w >> 2, cpr) + (w & 3)];
}

// fp32 rows -> sign bits: ailego::BinaryQuantizer::encode (src/ailego/algorithm/binary_quantizer.cc:40-57) into a zeroed row of
// ceil(dim / 32) words — bit i of a row is in[i] >= threshold for i < encode_dims (LSB first), every other bit of the row's words 0.
// What BinaryConverter does to the rows of an index (encode_dims = the converter's half, binary_converter.cc:69-73) and
// BinaryReformer to every query (encode_dims = dim, binary_reformer.cc:46-68).
//
// A streaming reader, 4 bytes in per bit out.  One wave per row at a time, a wave instruction per 64 consecutive values: lane l
// loads value 64 g + l (256 contiguous bytes per load; dword loads, so a row needs no more than its natural 4-byte alignment), the
// wave's ballot of the comparison IS words 2 g and 2 g + 1.  BENC_GROUPS loads are issued before the first ballot; their up to
// 2 * BENC_GROUPS words leave in one store of the first lanes.  The comparison is the plain fp32 one: -0 >= 0, nan never, denormals
// by their value (fp32 denormals are not flushed on gfx950).
constexpr int BENC_GROUPS = 4;
__global__ void __launch_bounds__(256) binary_encode_kernel(const float *in, uint64_t count, uint32_t dim, uint32_t encode_dims, float threshold,
                                                            uint32_t *out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t words = (dim + 31) / 32, groups = (words + 1) / 2;
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < count; row += (uint64_t)gridDim.x * 4) {
    const float *src = in + (size_t)row * dim;
    uint32_t *dst = out + (size_t)row * words;
    for (uint32_t g0 = 0; g0 < groups; g0 += BENC_GROUPS) {
      float v[BENC_GROUPS];
      bool in_range[BENC_GROUPS];
#pragma unroll
      for (int u = 0; u < BENC_GROUPS; ++u) {
        const uint32_t i = (g0 + u) * 64 + lane;
        in_range[u] = i < encode_dims;                 // (encode_dims <= dim: nothing beyond the row is read)
        v[u] = in_range[u] ? src[i] : 0.f;
      }
      uint32_t mine = 0;
#pragma unroll
      for (int u = 0; u < BENC_GROUPS; ++u) {
        const uint64_t m = __ballot(in_range[u] && v[u] >= threshold);
        if (lane == 2u * u) mine = (uint32_t)m;
        if (lane == 2u * u + 1) mine = (uint32_t)(m >> 32);
      }
      const uint32_t w = g0 * 2 + lane;
      if (lane < 2 * BENC_GROUPS && w < words) dst[w] = mine;
    }
  }
}

}  // namespace zvk
