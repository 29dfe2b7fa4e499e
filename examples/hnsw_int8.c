/* hnsw_int8.c — an HNSW index of int8 rows through the C ABI (zvec_hip_hnsw_create_typed with ZVEC_HIP_DT_INT8): fp32 rows are
 * quantised on the device (zvec_hip_int8_encode), 400 rows of 128 values are built on the device, 100 more are appended, and one
 * batch of queries is searched and checked against a brute-force integer loop.  The score is the squared distance as an exact
 * 32-bit integer, converted to float.  At ef = n the walk visits every node it can reach, so on a connected graph its answer is the
 * exact one.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_int8 examples/hnsw_int8.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zvec_hip.h"

#define N 500
#define BUILT 400
#define DIM 128
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

static float raw[N + NQ][DIM];
static int8_t rows[N + NQ][DIM];               /* the last NQ are the queries */
static uint64_t keys[N];

static float l2(const int8_t *a, const int8_t *b) {
  int32_t sum = 0;
  for (int k = 0; k < DIM; ++k) sum += ((int32_t)a[k] - b[k]) * ((int32_t)a[k] - b[k]);
  return (float)sum;
}

/* one batch at ef = n against a brute-force loop over the first n rows */
static int search_and_check(zvec_hip_hnsw_t h, int n) {
  static uint64_t out_keys[NQ][TOPK];
  static float out_scores[NQ][TOPK];
  static uint32_t out_counts[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &rows[N][0], NQ, TOPK, (uint32_t)n, 0, FLT_MAX, NULL, &out_keys[0][0], &out_scores[0][0], out_counts));
  for (int q = 0; q < NQ; ++q) {
    static float d[N];
    for (int i = 0; i < n; ++i) d[i] = l2(rows[N + q], rows[i]);
    if (out_counts[q] != TOPK) {
      printf("n %d query %d: %u results\n", n, q, out_counts[q]);
      return 1;
    }
    for (int j = 0; j < TOPK; ++j) {               /* the j-th smallest distance, by selection */
      int best = 0;
      for (int i = 1; i < n; ++i)
        if (d[i] < d[best]) best = i;
      const uint64_t pos = out_keys[q][j] - 1000u;
      if (out_scores[q][j] != d[best] || pos >= (uint64_t)n || l2(rows[N + q], rows[pos]) != d[best]) {
        printf("n %d query %d place %d: score %g, brute force %g\n", n, q, j, out_scores[q][j], d[best]);
        return 1;
      }
      d[best] = FLT_MAX;
    }
  }
  return 0;
}

int main(void) {
  /* 20 random centres in [-1, 1); a row or a query is a centre plus noise of a tenth of that, so that near neighbours exist */
  static float centres[20][DIM];
  uint32_t seed = 2026u;
  for (int c = 0; c < 20; ++c)
    for (int k = 0; k < DIM; ++k) {
      seed = seed * 1664525u + 1013904223u;
      centres[c][k] = (float)(seed >> 8) / 8388608.0f - 1.0f;
    }
  for (int i = 0; i < N + NQ; ++i)
    for (int k = 0; k < DIM; ++k) {
      seed = seed * 1664525u + 1013904223u;
      raw[i][k] = centres[i % 20][k] + ((float)(seed >> 8) / 8388608.0f - 1.0f) * 0.1f;
    }
  for (int i = 0; i < N; ++i) keys[i] = 1000u + (uint64_t)i;

  /* rows and queries through the quantiser with one scale: values within +-1.1 map onto +-110 */
  zvec_hip_ctx_t ctx = NULL;
  CHECK(zvec_hip_ctx_create(0, &ctx));
  CHECK(zvec_hip_int8_encode(ctx, &raw[0][0], N + NQ, DIM, ZVEC_HIP_INT8_SCALE_BIAS, 100.0f, 0.0f, &rows[0][0], NULL));
  CHECK(zvec_hip_ctx_destroy(ctx));

  zvec_hip_hnsw_t h = NULL;
  if (zvec_hip_hnsw_create(DIM, ZVEC_HIP_DT_INT8, ZVEC_HIP_METRIC_L2, 0, &h) != ZVEC_HIP_ERR_UNSUPPORTED || h != NULL ||
      zvec_hip_hnsw_create_typed(DIM + 2, ZVEC_HIP_DT_INT8, ZVEC_HIP_METRIC_L2, 0, &h) != ZVEC_HIP_ERR_INVALID_ARGUMENT || h != NULL) {
    printf("a creator took what it refuses\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_create_typed(DIM, ZVEC_HIP_DT_INT8, ZVEC_HIP_METRIC_L2, 0, &h));
  int dtype = -1;
  uint32_t dim = 0;
  CHECK(zvec_hip_hnsw_dtype(h, &dtype));
  CHECK(zvec_hip_hnsw_info(h, NULL, &dim, NULL, NULL, NULL, NULL, NULL));
  if (dtype != ZVEC_HIP_DT_INT8 || dim != DIM) {
    printf("dtype %d, dim %u\n", dtype, dim);
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
  /* the stored rows come back as the bytes that went in */
  static int8_t back[N][DIM];
  static uint64_t pos[N];
  for (int i = 0; i < N; ++i) pos[i] = (uint64_t)i;
  CHECK(zvec_hip_hnsw_get_vectors(h, pos, N, &back[0][0]));
  if (memcmp(back, rows, sizeof(back)) != 0) {
    printf("get_vectors differs\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  printf("hnsw_int8 ok\n");
  return 0;
}
