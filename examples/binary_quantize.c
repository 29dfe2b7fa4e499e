/* examples/binary_quantize.c — fp32 embeddings on a binary (sign-bit) index from plain C: create a flat Hamming index of
 * 32 * ceil(DIM / 32) bits, append fp32 documents (the library turns them into sign bits on the GPU, as BinaryConverter does in
 * front of an index), search with fp32 queries (BinaryReformer + search), print keys and scores and check every returned score
 * (and the best one of every query) against an encode + popcount loop in this file.
 *   gcc -std=c99 -Iinclude -o binary_quantize examples/binary_quantize.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 * Needs an MI355X at run time (there is no CPU fallback: zvec_hip_flat_create fails without a HIP device). */
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

enum { DIM = 100, WORDS = (DIM + 31) / 32, N = 1000, NQ = 3, K = 5 };

static float next_value(uint64_t *state) {            /* splitmix64 -> a value in [-1, 1) */
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (float)((z ^ (z >> 31)) >> 40) / 8388608.0f - 1.0f;
}

/* BinaryQuantizer::encode into a zeroed row: bit i = in[i] >= threshold, LSB first */
static void encode(const float *in, float threshold, uint32_t *out) {
  for (int w = 0; w < WORDS; ++w) out[w] = 0;
  for (int i = 0; i < DIM; ++i)
    if (in[i] >= threshold) out[i / 32] |= 1u << (i % 32);
}

static uint32_t hamming(const uint32_t *a, const uint32_t *b) {
  uint32_t d = 0;
  for (int w = 0; w < WORDS; ++w)
    for (uint32_t x = a[w] ^ b[w]; x; x &= x - 1) ++d;
  return d;
}

int main(void) {
  const float bin_threshold = 0.0f;
  zvec_hip_flat_t index = NULL;
  int rc = zvec_hip_flat_create(WORDS * 32, ZVEC_HIP_DT_BINARY32, ZVEC_HIP_METRIC_HAMMING, 0, &index);
  if (rc != 0) {
    fprintf(stderr, "zvec_hip_flat_create: %d (%s)\n", rc, zvec_hip_error_string(rc));
    return 1;
  }
  float *docs = (float *)malloc(sizeof(float) * DIM * N);
  uint32_t *bits = (uint32_t *)malloc(sizeof(uint32_t) * WORDS * N);
  uint64_t state = 11;
  for (int i = 0; i < N * DIM; ++i) docs[i] = next_value(&state);
  for (int i = 0; i < N; ++i) encode(docs + i * DIM, bin_threshold, bits + i * WORDS);
  /* all DIM values of a document are encoded (encode_dims = DIM); keys = storage positions */
  if ((rc = zvec_hip_flat_append_fp32(index, docs, N, DIM, DIM, bin_threshold, NULL)) != 0) return 2;
  uint32_t stored[WORDS];
  if ((rc = zvec_hip_flat_get_vector(index, 123, stored)) != 0) return 3;
  int bad = hamming(stored, bits + 123 * WORDS) != 0;
  float queries[NQ * DIM];
  uint32_t qbits[NQ * WORDS];
  for (int q = 0; q < NQ; ++q) {                        /* document 100 (q + 1) with the signs of its first q + 1 values flipped */
    for (int i = 0; i < DIM; ++i) queries[q * DIM + i] = docs[100 * (q + 1) * DIM + i];
    for (int b = 0; b <= q; ++b) queries[q * DIM + b] = queries[q * DIM + b] >= bin_threshold ? -1.0f : 1.0f;
    encode(queries + q * DIM, bin_threshold, qbits + q * WORDS);
  }
  uint64_t keys[NQ * K];
  float scores[NQ * K];
  uint32_t counts[NQ];
  rc = zvec_hip_flat_search_fp32(index, NULL, queries, DIM, bin_threshold, NQ, K, 3.4e38f, NULL, keys, scores, counts);
  if (rc != 0) return 4;
  for (int q = 0; q < NQ; ++q) {
    uint32_t best = WORDS * 32 + 1;
    for (uint32_t i = 0; i < N; ++i) {
      const uint32_t d = hamming(bits + i * WORDS, qbits + q * WORDS);
      if (d < best) best = d;
    }
    printf("query %d:", q);
    if (counts[q] != K) bad = 1;
    for (uint32_t j = 0; j < counts[q]; ++j) {
      const uint64_t key = keys[q * K + j];
      printf(" (%llu, %.0f)", (unsigned long long)key, scores[q * K + j]);
      if (key >= N || scores[q * K + j] != (float)hamming(bits + key * WORDS, qbits + q * WORDS)) bad = 1;
      if (j > 0 && scores[q * K + j] < scores[q * K + j - 1]) bad = 1;
    }
    printf("\n");
    if (counts[q] == 0 || scores[q * K] != (float)best || best != (uint32_t)(q + 1) || keys[q * K] != (uint64_t)(100 * (q + 1))) bad = 1;
  }
  free(docs);
  free(bits);
  zvec_hip_flat_destroy(index);
  return bad ? 5 : 0;
}
