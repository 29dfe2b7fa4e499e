/* hnsw_hamming.c — an HNSW index of binary rows under the Hamming distance through the C ABI (zvec_hip_hnsw_create_binary with
 * ZVEC_HIP_DT_BINARY32): 400 rows of 768 bits are built on the device, 100 more are appended, and one batch of queries is searched
 * and checked against a brute-force popcount loop.  A row is 24 uint32_t words; the score is (float) popcount(row ^ query), an exact
 * integer.  At ef = n the walk visits every node it can reach, so on a connected graph its answer is the exact one.
 *
 *   gcc -std=c99 -Iinclude -o hnsw_hamming examples/hnsw_hamming.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 */
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "zvec_hip.h"

#define N 500
#define BUILT 400
#define BITS 768
#define WORDS (BITS / 32)
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

static uint32_t rows[N][WORDS], queries[NQ][WORDS];
static uint64_t keys[N];

static float hamming(const uint32_t *a, const uint32_t *b) {
  int bits = 0;
  for (int k = 0; k < WORDS; ++k)
    for (uint32_t x = a[k] ^ b[k]; x != 0; x &= x - 1) ++bits;
  return (float)bits;
}

/* one batch at ef = n against a brute-force loop over the first n rows */
static int search_and_check(zvec_hip_hnsw_t h, int n) {
  static uint64_t out_keys[NQ][TOPK];
  static float out_scores[NQ][TOPK];
  static uint32_t out_counts[NQ];
  CHECK(zvec_hip_hnsw_search(h, NULL, &queries[0][0], NQ, TOPK, (uint32_t)n, 0, FLT_MAX, NULL, &out_keys[0][0], &out_scores[0][0], out_counts));
  for (int q = 0; q < NQ; ++q) {
    static float d[N];
    for (int i = 0; i < n; ++i) d[i] = hamming(queries[q], rows[i]);
    if (out_counts[q] != TOPK) {
      printf("n %d query %d: %u results\n", n, q, out_counts[q]);
      return 1;
    }
    for (int j = 0; j < TOPK; ++j) {               /* the j-th smallest distance, by selection */
      int best = 0;
      for (int i = 1; i < n; ++i)
        if (d[i] < d[best]) best = i;
      const uint64_t pos = out_keys[q][j] - 1000u;
      if (out_scores[q][j] != d[best] || pos >= (uint64_t)n || hamming(queries[q], rows[pos]) != d[best]) {
        printf("n %d query %d place %d: score %g, brute force %g\n", n, q, j, out_scores[q][j], d[best]);
        return 1;
      }
      d[best] = FLT_MAX;
    }
  }
  return 0;
}

int main(void) {
  /* 20 random centres; a row or a query is a centre with 60 of its bits flipped, so that near neighbours exist */
  static uint32_t centres[20][WORDS];
  uint32_t seed = 2026u;
  for (int c = 0; c < 20; ++c)
    for (int k = 0; k < WORDS; ++k) {
      seed = seed * 1664525u + 1013904223u;
      centres[c][k] = seed ^ (seed >> 13);
    }
  for (int i = 0; i < N + NQ; ++i) {
    uint32_t *row = i < N ? rows[i] : queries[i - N];
    memcpy(row, centres[i % 20], sizeof(centres[0]));
    for (int f = 0; f < 60; ++f) {
      seed = seed * 1664525u + 1013904223u;
      const uint32_t bit = (seed >> 8) % BITS;
      row[bit / 32] ^= 1u << (bit % 32);
    }
  }
  for (int i = 0; i < N; ++i) keys[i] = 1000u + (uint64_t)i;

  zvec_hip_hnsw_t h = NULL;
  if (zvec_hip_hnsw_create_typed(BITS, ZVEC_HIP_DT_BINARY32, ZVEC_HIP_METRIC_HAMMING, 0, &h) != ZVEC_HIP_ERR_UNSUPPORTED || h != NULL ||
      zvec_hip_hnsw_create_binary(BITS + 16, ZVEC_HIP_DT_BINARY32, 0, &h) != ZVEC_HIP_ERR_INVALID_ARGUMENT || h != NULL) {
    printf("a creator took what it refuses\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_create_binary(BITS, ZVEC_HIP_DT_BINARY32, 0, &h));
  int dtype = -1;
  uint32_t dim = 0;
  CHECK(zvec_hip_hnsw_dtype(h, &dtype));
  CHECK(zvec_hip_hnsw_info(h, NULL, &dim, NULL, NULL, NULL, NULL, NULL));
  if (dtype != ZVEC_HIP_DT_BINARY32 || dim != BITS) {
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
  /* the stored rows come back as the words that went in */
  static uint32_t back[N][WORDS];
  static uint64_t pos[N];
  for (int i = 0; i < N; ++i) pos[i] = (uint64_t)i;
  CHECK(zvec_hip_hnsw_get_vectors(h, pos, N, &back[0][0]));
  if (memcmp(back, rows, sizeof(rows)) != 0) {
    printf("get_vectors differs\n");
    return 1;
  }
  CHECK(zvec_hip_hnsw_destroy(h));
  printf("hnsw_hamming ok\n");
  return 0;
}
