/* examples/hamming_ivf_rerank.c — fp32 embeddings on a Hamming IVF index from plain C: build 8 inverted lists over documents of
 * 100 fp32 values (the library turns them into sign bits on the GPU, trains the lists on the bits and keeps the fp32 rows beside
 * them in list order), search one batch of fp32 queries with refine 4 (4 * K Hamming candidates per query, re-ranked on the fp32
 * rows by squared L2 without leaving the device), print keys and scores and check the result against an encode + popcount +
 * re-score loop in this file, restricted to the candidates read back.
 *   gcc -std=c99 -Iinclude -o hamming_ivf_rerank examples/hamming_ivf_rerank.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 * Needs an MI355X at run time (there is no CPU fallback: zvec_hip_bivf_create fails without a HIP device). */
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

enum { DIM = 100, WORDS = (DIM + 31) / 32, N = 2000, NLIST = 8, NQ = 4, K = 5, REFINE = 4, KC = K * REFINE, NPROBE = 3 };

static float next_value(uint64_t *state) {            /* splitmix64 -> a multiple of 1/8 in [-1, 1): every fp32 sum below is exact */
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (float)((int)((z ^ (z >> 31)) >> 60) - 8) / 8.0f;
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

static float l2(const float *a, const float *b) {
  float s = 0.0f;
  for (int i = 0; i < DIM; ++i) s += (a[i] - b[i]) * (a[i] - b[i]);
  return s;
}

int main(void) {
  const float bin_threshold = 0.0f;
  zvec_hip_bivf_t index = NULL;
  int rc = zvec_hip_bivf_create(WORDS * 32, ZVEC_HIP_DT_BINARY32, 0, &index);
  if (rc != 0) {
    fprintf(stderr, "zvec_hip_bivf_create: %d (%s)\n", rc, zvec_hip_error_string(rc));
    return 1;
  }
  float *docs = (float *)malloc(sizeof(float) * DIM * N);
  uint64_t *row_of = (uint64_t *)malloc(sizeof(uint64_t) * N);
  uint64_t state = 23;
  for (int i = 0; i < N * DIM; ++i) docs[i] = next_value(&state);
  /* keys = original row numbers; 10 k-means iterations on the bits */
  if ((rc = zvec_hip_bivf_build_fp32(index, docs, N, DIM, ZVEC_HIP_METRIC_L2, NULL, NLIST, 10, 7, bin_threshold)) != 0) return 2;
  if ((rc = zvec_hip_bivf_export(index, NULL, NULL, row_of)) != 0) return 3;
  /* the fp32 rows are in list order: position 17 holds document row_of[17] */
  float stored[DIM];
  const uint64_t probe_pos = 17;
  if ((rc = zvec_hip_bivf_get_rows(index, &probe_pos, 1, stored)) != 0) return 4;
  int bad = l2(stored, docs + row_of[17] * DIM) != 0.0f;
  float queries[NQ * DIM];
  for (int q = 0; q < NQ; ++q)                          /* document 300 (q + 1) with its first q + 1 values negated */
    for (int i = 0; i < DIM; ++i) queries[q * DIM + i] = (i <= q ? -1.0f : 1.0f) * docs[300 * (q + 1) * DIM + i];
  uint64_t keys[NQ * K];
  float scores[NQ * K];
  uint32_t counts[NQ];
  rc = zvec_hip_bivf_search_fp32(index, NULL, queries, NQ, DIM, K, REFINE, 3.4e38f, bin_threshold, NPROBE, 0xffffffffu, NULL, keys, scores,
                                 counts);
  if (rc != 0) return 5;
  uint32_t cand[NQ * KC], ccnt[NQ];
  float cham[NQ * KC];
  if ((rc = zvec_hip_bivf_last_candidates(index, NULL, NQ, KC, cand, cham, ccnt)) != 0) return 6;
  for (int q = 0; q < NQ; ++q) {
    uint32_t qbits[WORDS], dbits[WORDS];
    float cs[KC];
    int taken[KC];
    encode(queries + q * DIM, bin_threshold, qbits);
    for (uint32_t c = 0; c < ccnt[q]; ++c) {            /* stage 1 as read back: Hamming scores exact and ascending */
      const float *doc = docs + row_of[cand[q * KC + c]] * DIM;
      encode(doc, bin_threshold, dbits);
      if (cham[q * KC + c] != (float)hamming(dbits, qbits) || (c > 0 && cham[q * KC + c] < cham[q * KC + c - 1])) bad = 1;
      cs[c] = l2(queries + q * DIM, doc);
      taken[c] = 0;
    }
    printf("query %d:", q);
    if (counts[q] != (ccnt[q] < K ? ccnt[q] : K)) bad = 1;
    for (uint32_t j = 0; j < counts[q]; ++j) {          /* stage 2: the j-th smallest by (score, rank) among the candidates */
      int best = -1;
      for (uint32_t c = 0; c < ccnt[q]; ++c)
        if (!taken[c] && (best < 0 || cs[c] < cs[best])) best = (int)c;
      taken[best] = 1;
      printf(" (%llu, %.4f)", (unsigned long long)keys[q * K + j], scores[q * K + j]);
      if (keys[q * K + j] != row_of[cand[q * KC + best]] || scores[q * K + j] != cs[best]) bad = 1;
    }
    printf("\n");
    /* the query's own document differs in q + 1 signs: where its list is probed it is a candidate, and then it wins the re-rank */
    int own = 0;
    for (uint32_t c = 0; c < ccnt[q]; ++c) own |= row_of[cand[q * KC + c]] == (uint64_t)(300 * (q + 1));
    if (counts[q] == 0 || (own && keys[q * K] != (uint64_t)(300 * (q + 1)))) bad = 1;
  }
  free(docs);
  free(row_of);
  zvec_hip_bivf_destroy(index);
  return bad ? 7 : 0;
}
