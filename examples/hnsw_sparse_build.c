/* Building a graph over sparse rows from plain C99 (zvec_hip_hnsw_sparse_build): 2000 documents of up to 24 (index, value) pairs go
 * in, the graph is built on the device in rounds, read back and checked for shape, then searched under InnerProductSparse; every
 * returned score is checked against a merge-join loop in this file.  Values are small integers, so every fp32 sum is exact.
 *   gcc -std=c99 -Iinclude examples/hnsw_sparse_build.c -Lzvec_amd -lzvec_hip -Wl,-rpath,zvec_amd */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

#define N 2000
#define NQ 8
#define TOPK 5
#define VOCAB 160
#define MAXC 24
#define M 8
#define M0 16

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
  static uint32_t qcounts[NQ], qoff[NQ + 1], qidx[NQ * MAXC];
  static float qval[NQ * MAXC];
  uint64_t out_keys[NQ * TOPK], n = 0, elements = 0;
  float out_scores[NQ * TOPK];
  uint32_t out_counts[NQ], i, q, j, m0 = 0;
  zvec_hip_hnsw_build_params p = {M, M0, 64, 0, 0, 0, 7};      /* prune_cnt and scaling_factor: the defaults (m) */
  zvec_hip_hnsw_build_info info;
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
  }
  for (q = 0; q < NQ; ++q) {
    qcounts[q] = 1 + rnd() % MAXC;
    qoff[q + 1] = qoff[q] + qcounts[q];
    make_run(qcounts[q], qidx + qoff[q], qval + qoff[q]);
  }

  CHECK(zvec_hip_hnsw_sparse_create(ZVEC_HIP_DT_FP32, ZVEC_HIP_METRIC_IP, 0, &h));
  if (zvec_hip_hnsw_sparse_last_build_info(h, &info) != ZVEC_HIP_ERR_NO_READY) {
    printf("build info before a build\n");
    return 1;
  }
  /* keys NULL: a document's key is its position; levels NULL: generated from the seed */
  CHECK(zvec_hip_hnsw_sparse_build(h, N, counts, idx, val, NULL, &p, NULL));
  CHECK(zvec_hip_hnsw_sparse_last_build_info(h, &info));
  CHECK(zvec_hip_hnsw_sparse_info(h, &n, &elements, &m0, NULL, NULL, NULL, NULL));
  if (n != N || elements != off[N] || m0 != M0 || info.rounds == 0 || info.requests == 0) {
    printf("unexpected shape: n %llu, elements %llu, m0 %u, rounds %u\n", (unsigned long long)n, (unsigned long long)elements, m0, info.rounds);
    return 1;
  }
  CHECK(zvec_hip_hnsw_sparse_export(h, NULL, nbr0, cnt0, NULL, NULL, NULL));
  for (i = 0; i < N; ++i) {
    if (cnt0[i] > M0) { printf("node %u: %u neighbours\n", i, cnt0[i]); return 1; }
    for (j = 0; j < cnt0[i]; ++j)
      if (nbr0[i * M0 + j] >= N || nbr0[i * M0 + j] == i) { printf("node %u: neighbour %u\n", i, nbr0[i * M0 + j]); return 1; }
  }

  CHECK(zvec_hip_hnsw_sparse_search(h, NULL, qcounts, qidx, qval, NQ, TOPK, 64, 0, 3.0e38f, NULL, out_keys, out_scores, out_counts));
  for (q = 0; q < NQ; ++q) {
    if (out_counts[q] != TOPK) {
      printf("query %u: %u results\n", q, out_counts[q]);
      return 1;
    }
    for (j = 0; j < TOPK; ++j) {
      const uint64_t k = out_keys[q * TOPK + j];
      if (k >= N || (j && out_scores[q * TOPK + j] < out_scores[q * TOPK + j - 1]) ||
          out_scores[q * TOPK + j] != score_of(idx + off[k], val + off[k], counts[k], qidx + qoff[q], qval + qoff[q], qcounts[q])) {
        printf("query %u place %u: key %llu score %g\n", q, j, (unsigned long long)k, out_scores[q * TOPK + j]);
        return 1;
      }
    }
  }
  CHECK(zvec_hip_hnsw_sparse_destroy(h));
  printf("hnsw_sparse_build ok: %d documents in %u rounds, %llu distances, %llu links asked for, %llu prunes; top %d of %d queries\n", N,
         info.rounds, (unsigned long long)info.dists, (unsigned long long)info.requests, (unsigned long long)info.prunes, TOPK, NQ);
  return 0;
}
