/* hnsw_search.c — search a hand-built graph through the C ABI (zvec_hip_hnsw_*): a ring of 64 nodes with chords, one batch of
 * queries, checked against a brute-force loop.  At ef = n every node of a connected graph is visited, so the walk's answer is the
 * exact one; integer rows make every fp32 distance exact.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_search examples/hnsw_search.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

#define N 64
#define DIM 8
#define M0 4
#define NQ 4
#define TOPK 5

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
  static uint32_t nbr0[N][M0], cnt0[N];
  uint32_t seed = 12345u;
  for (int i = 0; i < N; ++i) {
    for (int d = 0; d < DIM; ++d) {
      seed = seed * 1664525u + 1013904223u;
      rows[i][d] = (float)((int)((seed >> 16) % 17u) - 8);
    }
    keys[i] = 1000u + (uint64_t)i;
    nbr0[i][0] = (uint32_t)((i + 1) % N);          /* the ring ... */
    nbr0[i][1] = (uint32_t)((i + N - 1) % N);
    nbr0[i][2] = (uint32_t)((i + 9) % N);          /* ... and two chords */
    nbr0[i][3] = (uint32_t)((i + 23) % N);
    cnt0[i] = M0;
  }
  for (int q = 0; q < NQ; ++q)
    for (int d = 0; d < DIM; ++d) {
      seed = seed * 1664525u + 1013904223u;
      queries[q][d] = (float)((int)((seed >> 16) % 17u) - 8);
    }

  zvec_hip_hnsw_t h;
  CHECK(zvec_hip_hnsw_create(DIM, ZVEC_HIP_DT_FP32, ZVEC_HIP_METRIC_L2, 0, &h));
  /* level 0 only: max_level = 0, no upper arrays; entry point 0 */
  CHECK(zvec_hip_hnsw_load(h, N, &rows[0][0], keys, M0, &nbr0[0][0], cnt0, 0, 0, 0, NULL, NULL, NULL, 0));

  uint64_t out_keys[NQ][TOPK];
  float out_scores[NQ][TOPK];
  uint32_t out_counts[NQ], scanned[NQ], hops[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &queries[0][0], NQ, TOPK, /*ef=*/N, /*max_scan=*/0, FLT_MAX, NULL, &out_keys[0][0],
                             &out_scores[0][0], out_counts));
  CHECK(zvec_hip_hnsw_last_stats(h, NULL, NQ, scanned, hops, NULL));

  int bad = 0;
  for (int q = 0; q < NQ; ++q) {
    /* brute force: the TOPK smallest by (distance, node) */
    float dist[N];
    int used[N] = {0};
    for (int i = 0; i < N; ++i) {
      float s = 0.f;
      for (int d = 0; d < DIM; ++d) s += (queries[q][d] - rows[i][d]) * (queries[q][d] - rows[i][d]);
      dist[i] = s;
    }
    printf("query %d (%u distances, %u nodes expanded):", q, scanned[q], hops[q]);
    if (out_counts[q] != TOPK) bad = 1;
    for (int j = 0; j < TOPK; ++j) {
      int best = -1;
      for (int i = 0; i < N; ++i)
        if (!used[i] && (best < 0 || dist[i] < dist[best])) best = i;
      used[best] = 1;
      printf(" %llu:%g", (unsigned long long)out_keys[q][j], out_scores[q][j]);
      if (out_keys[q][j] != keys[best] || out_scores[q][j] != dist[best]) bad = 1;
    }
    printf("\n");
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  if (bad) {
    printf("hnsw_search MISMATCH against brute force\n");
    return 1;
  }
  printf("hnsw_search ok\n");
  return 0;
}
