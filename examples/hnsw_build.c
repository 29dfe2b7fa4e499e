/* hnsw_build.c — rows in, graph out, through the C ABI (zvec_hip_hnsw_build): 400 rows are inserted in rounds on the device, then
 * one batch of queries is searched on the built graph and checked against a brute-force loop.  At ef = n the walk visits every
 * node it can reach, so on a connected graph its answer is the exact one; integer rows make every fp32 distance exact.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_build examples/hnsw_build.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zvec_hip.h"

#define N 400
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

int main(void) {
  static float rows[N][DIM], queries[NQ][DIM];
  static uint64_t keys[N];
  uint32_t seed = 2024u;
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
  zvec_hip_hnsw_build_params p;
  memset(&p, 0, sizeof(p));                      /* a field left 0 takes the reference's default */
  p.m = 8;                                       /* m0 = 16, prune_cnt = 8, scaling_factor = 8 */
  p.ef_construction = 64;
  p.seed = 7;
  CHECK(zvec_hip_hnsw_build(h, N, &rows[0][0], keys, &p, NULL));      /* NULL: the levels are generated from the seed */
  zvec_hip_hnsw_build_info bi;
  CHECK(zvec_hip_hnsw_last_build_info(h, &bi));
  uint64_t n = 0;
  uint32_t m0 = 0, max_level = 0, entry = 0;
  CHECK(zvec_hip_hnsw_info(h, &n, NULL, &m0, &max_level, NULL, NULL, &entry));
  printf("built %llu nodes in %u rounds: m0 %u, top level %u, entry point %u; %llu distances, %llu requests, %llu prunes\n",
         (unsigned long long)n, bi.rounds, m0, max_level, entry, (unsigned long long)bi.dists, (unsigned long long)bi.requests,
         (unsigned long long)bi.prunes);
  if (n != N || m0 != 16 || bi.top != max_level || bi.entry_point != entry || bi.requests == 0) {
    printf("unexpected shape\n");
    return 1;
  }

  static uint64_t out_keys[NQ][TOPK];
  static float out_scores[NQ][TOPK];
  static uint32_t out_counts[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &queries[0][0], NQ, TOPK, N, 0, FLT_MAX, NULL, &out_keys[0][0], &out_scores[0][0], out_counts));
  for (int q = 0; q < NQ; ++q) {
    float d[N];
    for (int i = 0; i < N; ++i) {
      d[i] = 0.f;
      for (int k = 0; k < DIM; ++k) d[i] += (queries[q][k] - rows[i][k]) * (queries[q][k] - rows[i][k]);
    }
    if (out_counts[q] != TOPK) {
      printf("query %d: %u results\n", q, out_counts[q]);
      return 1;
    }
    for (int j = 0; j < TOPK; ++j) {               /* the j-th smallest distance, by selection */
      int best = 0;
      for (int i = 1; i < N; ++i)
        if (d[i] < d[best]) best = i;
      const uint64_t pos = out_keys[q][j] - 1000u;
      if (out_scores[q][j] != d[best] || pos >= N) {
        printf("query %d place %d: score %g, brute force %g\n", q, j, out_scores[q][j], d[best]);
        return 1;
      }
      float own = 0.f;
      for (int k = 0; k < DIM; ++k) own += (queries[q][k] - rows[pos][k]) * (queries[q][k] - rows[pos][k]);
      if (own != out_scores[q][j]) {
        printf("query %d place %d: key %llu is not at its score\n", q, j, (unsigned long long)out_keys[q][j]);
        return 1;
      }
      d[best] = FLT_MAX;
    }
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  printf("hnsw_build ok\n");
  return 0;
}
