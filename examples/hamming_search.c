/* examples/hamming_search.c — binary vectors under the Hamming metric from plain C: create a flat index of 256-bit rows, add
 * documents the way the product does (one add-with-id call per document), search a small batch, print keys and scores and
 * check every returned score (and the best one of every query) against a popcount loop in this file.
 *   gcc -std=c99 -Iinclude -o hamming_search examples/hamming_search.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 * Needs an MI355X at run time (there is no CPU fallback: zvec_hip_flat_create fails without a HIP device). */
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

enum { BITS = 256, WORDS = BITS / 32, N = 1000, NQ = 3, K = 5 };

static uint32_t next_word(uint64_t *state) {          /* splitmix64, upper half */
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static uint32_t hamming(const uint32_t *a, const uint32_t *b) {
  uint32_t d = 0;
  for (int w = 0; w < WORDS; ++w)
    for (uint32_t x = a[w] ^ b[w]; x; x &= x - 1) ++d;
  return d;
}

int main(void) {
  zvec_hip_flat_t index = NULL;
  int rc = zvec_hip_flat_create(BITS, ZVEC_HIP_DT_BINARY32, ZVEC_HIP_METRIC_HAMMING, 0, &index);
  if (rc != 0) {
    fprintf(stderr, "zvec_hip_flat_create: %d (%s)\n", rc, zvec_hip_error_string(rc));
    return 1;
  }
  uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * WORDS * N);
  uint64_t state = 7;
  for (uint32_t id = 0; id < N; ++id) {
    for (int w = 0; w < WORDS; ++w) rows[id * WORDS + w] = next_word(&state);
    if ((rc = zvec_hip_flat_put(index, &id, 1, rows + id * WORDS, NULL)) != 0) return 2;
  }
  uint32_t queries[NQ * WORDS];
  for (int q = 0; q < NQ; ++q) {                        /* document 100 (q + 1) with q + 1 bits flipped */
    for (int w = 0; w < WORDS; ++w) queries[q * WORDS + w] = rows[100 * (q + 1) * WORDS + w];
    for (int b = 0; b <= q; ++b) queries[q * WORDS + b] ^= 1u << (3 * b);
  }
  uint64_t keys[NQ * K];
  float scores[NQ * K];
  uint32_t counts[NQ];
  rc = zvec_hip_flat_search(index, NULL, queries, NQ, K, 3.4e38f, NULL, keys, scores, counts);
  if (rc != 0) return 3;
  int bad = 0;
  for (int q = 0; q < NQ; ++q) {
    uint32_t best = BITS + 1;
    for (uint32_t i = 0; i < N; ++i) {
      const uint32_t d = hamming(rows + i * WORDS, queries + q * WORDS);
      if (d < best) best = d;
    }
    printf("query %d:", q);
    if (counts[q] != K) bad = 1;
    for (uint32_t j = 0; j < counts[q]; ++j) {
      const uint64_t key = keys[q * K + j];
      printf(" (%llu, %.0f)", (unsigned long long)key, scores[q * K + j]);
      if (key >= N || scores[q * K + j] != (float)hamming(rows + key * WORDS, queries + q * WORDS)) bad = 1;
      if (j > 0 && scores[q * K + j] < scores[q * K + j - 1]) bad = 1;
    }
    printf("\n");
    if (counts[q] == 0 || scores[q * K] != (float)best || keys[q * K] != (uint64_t)(100 * (q + 1))) bad = 1;
  }
  free(rows);
  zvec_hip_flat_destroy(index);
  return bad ? 4 : 0;
}
