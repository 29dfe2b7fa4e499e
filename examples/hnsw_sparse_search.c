/* A graph over sparse rows from plain C99 (zvec_hip_hnsw_sparse_*): 300 documents of up to 24 (index, value) pairs, a ring with
 * chords built by hand, one batch search under InnerProductSparse at ef = n, checked against a merge-join loop in this file.
 * Values are small integers, so every fp32 sum is exact; ties are ordered by (score, position), as the library orders them.
 *   gcc -std=c99 -Iinclude examples/hnsw_sparse_search.c -Lzvec_amd -lzvec_hip -Wl,-rpath,zvec_amd */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

#define N 300
#define NQ 8
#define TOPK 5
#define VOCAB 160
#define MAXC 24
#define M0 5

static uint32_t rnd_state = 12345u;
static uint32_t rnd(void) {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

/* a run of `count` strictly ascending indices below VOCAB with values in -4 .. 4 without 0 */
static void make_run(uint32_t count, uint32_t *idx, float *val) {
  uint32_t at = 0, left = count, i;
  for (i = 0; i < VOCAB && left; ++i)
    if (rnd() % (VOCAB - i) < left) {
      int v = (int)(rnd() % 8) - 4;
      idx[at] = i;
      val[at++] = (float)(v >= 0 ? v + 1 : v);
      --left;
    }
}

/* MinusInnerProductSparseMatrix::Compute: a merge join of two ascending runs */
static float score_of(const uint32_t *ai, const float *av, uint32_t an, const uint32_t *bi, const float *bv, uint32_t bn) {
  float s = 0.f;
  uint32_t a = 0, b = 0;
  while (a < an && b < bn) {
    if (ai[a] < bi[b]) ++a;
    else if (ai[a] > bi[b]) ++b;
    else s += av[a++] * bv[b++];
  }
  return 0.f - s;
}

#define CHECK(call)                                                   \
  do {                                                                \
    int rc_ = (call);                                                 \
    if (rc_ != 0) {                                                   \
      printf("%s failed: %d (%s)\n", #call, rc_, zvec_hip_error_string(rc_)); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main(void) {
  static uint32_t counts[N], off[N + 1], idx[N * MAXC], nbr0[N * M0], cnt0[N];
  static float val[N * MAXC];
  static uint64_t keys[N];
  static uint32_t qcounts[NQ], qoff[NQ + 1], qidx[NQ * MAXC];
  static float qval[NQ * MAXC];
  uint64_t out_keys[NQ * TOPK];
  float out_scores[NQ * TOPK];
  uint32_t out_counts[NQ], i, q, j;
  const int chords[M0] = {1, -1, 7, 16, 61};
  zvec_hip_hnsw_sparse_t h = NULL;
  int dev = 0;

  if (zvec_hip_device_count(&dev) != 0 || dev == 0) {
    printf("no HIP device\n");
    return 1;
  }
  for (i = 0; i < N; ++i) {
    counts[i] = i % 37 == 0 ? 0 : 1 + rnd() % MAXC;          /* a few empty documents */
    off[i + 1] = off[i] + counts[i];
    make_run(counts[i], idx + off[i], val + off[i]);
    keys[i] = 3 * (uint64_t)i + 1;
    cnt0[i] = M0;
    for (j = 0; j < M0; ++j) nbr0[i * M0 + j] = (uint32_t)((int)(i + N) + chords[j]) % N;
  }
  for (q = 0; q < NQ; ++q) {
    qcounts[q] = q == 0 ? 0 : 1 + rnd() % MAXC;              /* and one empty query */
    qoff[q + 1] = qoff[q] + qcounts[q];
    make_run(qcounts[q], qidx + qoff[q], qval + qoff[q]);
  }

  CHECK(zvec_hip_hnsw_sparse_create(ZVEC_HIP_DT_FP32, ZVEC_HIP_METRIC_IP, 0, &h));
  CHECK(zvec_hip_hnsw_sparse_load(h, N, counts, idx, val, keys, M0, nbr0, cnt0, 0, 0, 0, NULL, NULL, NULL, 0));
  /* ef = n: the walk reaches every node of the ring, so the answer is the exact one */
  CHECK(zvec_hip_hnsw_sparse_search(h, NULL, qcounts, qidx, qval, NQ, TOPK, N, 0, 3.0e38f, NULL, out_keys, out_scores, out_counts));

  for (q = 0; q < NQ; ++q) {
    float best_s[TOPK];
    uint32_t best_i[TOPK], have = 0;
    for (i = 0; i < N; ++i) {                                 /* the TOPK smallest by (score, position), by insertion */
      const float s = score_of(idx + off[i], val + off[i], counts[i], qidx + qoff[q], qval + qoff[q], qcounts[q]);
      uint32_t p = have < TOPK ? have : TOPK;
      while (p > 0 && best_s[p - 1] > s) {
        if (p < TOPK) { best_s[p] = best_s[p - 1]; best_i[p] = best_i[p - 1]; }
        --p;
      }
      if (p < TOPK) { best_s[p] = s; best_i[p] = i; }
      if (have < TOPK) ++have;
    }
    if (out_counts[q] != TOPK) {
      printf("query %u: %u results\n", q, out_counts[q]);
      return 1;
    }
    for (j = 0; j < TOPK; ++j)
      if (out_keys[q * TOPK + j] != keys[best_i[j]] || out_scores[q * TOPK + j] != best_s[j]) {
        printf("query %u place %u: key %llu score %g, expected key %llu score %g\n", q, j, (unsigned long long)out_keys[q * TOPK + j],
               out_scores[q * TOPK + j], (unsigned long long)keys[best_i[j]], best_s[j]);
        return 1;
      }
  }
  CHECK(zvec_hip_hnsw_sparse_destroy(h));
  printf("hnsw_sparse_search ok: %d queries, top %d of %d sparse documents\n", NQ, TOPK, N);
  return 0;
}
