/* hnsw_append.c — rows arrive after the index exists, through the C ABI (zvec_hip_hnsw_add): 300 rows are built on the device, then
 * 100 more are appended in calls of 1, 9 and 90 rows, and after every call one batch of queries is searched and checked against a
 * brute-force loop over the rows the graph holds at that moment.  At ef = n the walk visits every node it can reach, so on a
 * connected graph its answer is the exact one; integer rows make every fp32 distance exact.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_append examples/hnsw_append.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zvec_hip.h"

#define N 400
#define BUILT 300
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

static float rows[N][DIM], queries[NQ][DIM];
static uint64_t keys[N];

/* one batch at ef = n against a brute-force loop over the first n rows */
static int search_and_check(zvec_hip_hnsw_t h, int n) {
  static uint64_t out_keys[NQ][TOPK];
  static float out_scores[NQ][TOPK];
  static uint32_t out_counts[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &queries[0][0], NQ, TOPK, (uint32_t)n, 0, FLT_MAX, NULL, &out_keys[0][0], &out_scores[0][0], out_counts));
  for (int q = 0; q < NQ; ++q) {
    float d[N];
    for (int i = 0; i < n; ++i) {
      d[i] = 0.f;
      for (int k = 0; k < DIM; ++k) d[i] += (queries[q][k] - rows[i][k]) * (queries[q][k] - rows[i][k]);
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
  uint32_t seed = 2025u;
  for (int i = 0; i < N; ++i) {
    for (int d = 0; d < DIM; ++d) {
      seed = seed * 1664525u + 1013904223u;
      rows[i][d] = (float)((int)((seed >> 16) % 17u) - 8);
    }
    keys[i] = 1000u + (uint64_t)i;
  }
  for (int q = 0; q < NQ; ++q)
    for (int d = 0; d < DIM; ++d) {
      seed = seed * 1664525u + 1013904223u;
      queries[q][d] = (float)((int)((seed >> 16) % 17u) - 8);
    }

  zvec_hip_hnsw_t h = NULL;
  CHECK(zvec_hip_hnsw_create(DIM, ZVEC_HIP_DT_FP32, ZVEC_HIP_METRIC_L2, 0, &h));
  zvec_hip_hnsw_add_info ai;
  if (zvec_hip_hnsw_last_add_info(h, &ai) != ZVEC_HIP_ERR_NO_READY) {
    printf("add info before the first add\n");
    return 1;
  }
  zvec_hip_hnsw_build_params p;
  memset(&p, 0, sizeof(p));                      /* a field left 0 takes the reference's default */
  p.m = 8;                                       /* m0 = 16, prune_cnt = 8, scaling_factor = 8 */
  p.ef_construction = 64;
  p.seed = 7;
  CHECK(zvec_hip_hnsw_build(h, BUILT, &rows[0][0], keys, &p, NULL));  /* NULL: the levels are generated from the seed */
  CHECK(zvec_hip_hnsw_reserve(h, N, 0));         /* room for all rows: the adds below move nothing */
  if (search_and_check(h, BUILT)) return 1;

  const int calls[3] = {1, 9, 90};
  int n = BUILT;
  for (int c = 0; c < 3; ++c) {
    /* NULL parameters: those of the build, its seed included, so the levels are those of one build of all rows */
    CHECK(zvec_hip_hnsw_add(h, (uint64_t)calls[c], &rows[n][0], keys + n, NULL, NULL));
    CHECK(zvec_hip_hnsw_last_add_info(h, &ai));
    uint64_t now = 0;
    CHECK(zvec_hip_hnsw_info(h, &now, NULL, NULL, NULL, NULL, NULL, NULL));
    printf("added %llu rows at %llu in %u rounds (%u of one node): %llu distances, %llu requests, %llu prunes; room for %llu rows\n",
           (unsigned long long)ai.count, (unsigned long long)ai.first, ai.rounds, ai.rounds_one, (unsigned long long)ai.dists,
           (unsigned long long)ai.requests, (unsigned long long)ai.prunes, (unsigned long long)ai.cap_rows);
    if (ai.first != (uint64_t)n || ai.count != (uint64_t)calls[c] || now != (uint64_t)(n + calls[c]) || ai.grew_rows || ai.requests == 0 ||
        ai.cap_rows != N || (calls[c] == 1 && ai.rounds_one != 1)) {
      printf("unexpected add info\n");
      return 1;
    }
    n += calls[c];
    if (search_and_check(h, n)) return 1;
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  printf("hnsw_append ok\n");
  return 0;
}
