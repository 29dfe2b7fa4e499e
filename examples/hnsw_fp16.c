/* hnsw_fp16.c — an HNSW index of IEEE binary16 rows through the C ABI (zvec_hip_hnsw_create_typed with ZVEC_HIP_DT_FP16): 400 rows of
 * small exactly representable values are built on the device, 100 more are appended, and one batch of binary16 queries is searched
 * and checked against a brute-force loop over the widened values.  The halves are made by a few lines of integer code (no compiler
 * half type is needed to use the interface).  At ef = n the walk visits every node it can reach, so on a connected graph its answer is
 * the exact one; the values are multiples of 1/4 below 8, so every fp32 distance is exact in any summation order.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_fp16 examples/hnsw_fp16.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zvec_hip.h"

#define N 500
#define BUILT 400
#define DIM 12
#define NQ 8
#define TOPK 10

#define CHECK(call)                                                                      \
  do {                                                                                   \
    int rc_ = (call);                                                                    \
    if (rc_ != 0) {                                                                      \
      printf("%s failed: %d (%s)\n", #call, rc_, zvec_hip_error_string(rc_));          \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

/* float -> IEEE binary16, round to nearest even; finite values inside the half range (subnormal results included) */
uint16_t half_of_float(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  const uint16_t sign = (uint16_t)((b >> 16) & 0x8000u);
  const int32_t e = (int32_t)((b >> 23) & 0xffu) - 127 + 15;       /* the half's biased exponent */
  uint32_t m = b & 0x7fffffu;
  if (((b >> 23) & 0xffu) == 0 || e < -10) return sign;            /* rounds to zero */
  uint32_t h, rest, halfway;
  if (e <= 0) {                                                    /* a subnormal half: the hidden bit moves into the fraction */
    m |= 0x800000u;
    const int shift = 14 - e;                                      /* 14 .. 24 */
    h = m >> shift;
    rest = m & ((1u << shift) - 1u);
    halfway = 1u << (shift - 1);
  } else {
    h = ((uint32_t)e << 10) | (m >> 13);
    rest = m & 0x1fffu;
    halfway = 0x1000u;
  }
  if (rest > halfway || (rest == halfway && (h & 1u))) ++h;        /* (a carry out of the fraction raises the exponent) */
  return (uint16_t)(sign | h);
}

/* IEEE binary16 -> float, exact */
float float_of_half(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu, b;
  if (e == 0) {
    if (m == 0) {
      b = sign;
    } else {                                                       /* subnormal: normalise */
      e = 1;
      while (!(m & 0x400u)) { m <<= 1; --e; }
      b = sign | ((e + 127 - 15) << 23) | ((m & 0x3ffu) << 13);
    }
  } else {
    b = sign | ((e + 127 - 15) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &b, 4);
  return f;
}

#ifndef HNSW_FP16_NO_MAIN
static uint16_t rows[N][DIM], queries[NQ][DIM];
static float wide_rows[N][DIM], wide_queries[NQ][DIM];             /* the widened values: what the brute-force loop reads */
static uint64_t keys[N];

/* one batch at ef = n against a brute-force loop over the first n rows */
static int search_and_check(zvec_hip_hnsw_t h, int n) {
  static uint64_t out_keys[NQ][TOPK];
  static float out_scores[NQ][TOPK];
  static uint32_t out_counts[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &queries[0][0], NQ, TOPK, (uint32_t)n, 0, FLT_MAX, NULL, &out_keys[0][0], &out_scores[0][0], out_counts));
  for (int q = 0; q < NQ; ++q) {
    static float d[N];
    for (int i = 0; i < n; ++i) {
      d[i] = 0.f;
      for (int k = 0; k < DIM; ++k) d[i] += (wide_queries[q][k] - wide_rows[i][k]) * (wide_queries[q][k] - wide_rows[i][k]);
    }
    if (out_counts[q] != TOPK) {
      printf("n %d query %d: %u results\n", n, q, out_counts[q]);
      return 1;
    }
    for (int j = 0; j < TOPK; ++j) {               /* the j-th smallest distance, by selection */
      int best = 0;
      for (int i = 1; i < n; ++i)
        if (d[i] < d[best]) best = i;
      const uint64_t pos = out_keys[q][j] - 1000u;
      if (out_scores[q][j] != d[best] || pos >= (uint64_t)n) {
        printf("n %d query %d place %d: score %g, brute force %g\n", n, q, j, out_scores[q][j], d[best]);
        return 1;
      }
      d[best] = FLT_MAX;
    }
  }
  return 0;
}

int main(void) {
  uint32_t seed = 2026u;
  for (int i = 0; i < N + NQ; ++i)
    for (int d = 0; d < DIM; ++d) {
      seed = seed * 1664525u + 1013904223u;
      const float v = (float)((int)((seed >> 16) % 65u) - 32) * 0.25f;       /* -8 .. 8 in steps of 1/4 */
      const uint16_t hv = half_of_float(v);
      if (float_of_half(hv) != v) {
        printf("%g is not a half\n", v);
        return 1;
      }
      if (i < N) { rows[i][d] = hv; wide_rows[i][d] = v; }
      else { queries[i - N][d] = hv; wide_queries[i - N][d] = v; }
    }
  for (int i = 0; i < N; ++i) keys[i] = 1000u + (uint64_t)i;

  zvec_hip_hnsw_t h = NULL;
  if (zvec_hip_hnsw_create(DIM, ZVEC_HIP_DT_FP16, ZVEC_HIP_METRIC_L2, 0, &h) != ZVEC_HIP_ERR_UNSUPPORTED || h != NULL) {
    printf("the fp32 creator took fp16\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_create_typed(DIM, ZVEC_HIP_DT_FP16, ZVEC_HIP_METRIC_L2, 0, &h));
  int dtype = -1;
  CHECK(zvec_hip_hnsw_dtype(h, &dtype));
  if (dtype != ZVEC_HIP_DT_FP16) {
    printf("dtype %d\n", dtype);
    return 1;
  }
  zvec_hip_hnsw_build_params p;
  memset(&p, 0, sizeof(p));                      /* a field left 0 takes the reference's default */
  p.m = 8;                                       /* m0 = 16, prune_cnt = 8, scaling_factor = 8 */
  p.ef_construction = 64;
  p.seed = 7;
  CHECK(zvec_hip_hnsw_build(h, BUILT, &rows[0][0], keys, &p, NULL));  /* NULL: the levels are generated from the seed */
  if (search_and_check(h, BUILT)) return 1;
  CHECK(zvec_hip_hnsw_add(h, N - BUILT, &rows[BUILT][0], keys + BUILT, NULL, NULL));      /* NULL parameters: those of the build */
  zvec_hip_hnsw_add_info ai;
  CHECK(zvec_hip_hnsw_last_add_info(h, &ai));
  printf("added %llu rows at %llu in %u rounds: %llu distances, %llu requests, %llu prunes\n", (unsigned long long)ai.count,
         (unsigned long long)ai.first, ai.rounds, (unsigned long long)ai.dists, (unsigned long long)ai.requests,
         (unsigned long long)ai.prunes);
  if (search_and_check(h, N)) return 1;
  /* the stored rows come back as the halves that went in */
  static uint16_t back[N][DIM];
  static uint64_t pos[N];
  for (int i = 0; i < N; ++i) pos[i] = (uint64_t)i;
  CHECK(zvec_hip_hnsw_get_vectors(h, pos, N, &back[0][0]));
  if (memcmp(back, rows, sizeof(rows)) != 0) {
    printf("get_vectors differs\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  printf("hnsw_fp16 ok\n");
  return 0;
}
#endif
