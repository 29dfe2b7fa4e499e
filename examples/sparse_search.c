/* examples/sparse_search.c — sparse vectors under InnerProductSparse from plain C: create a flat index of sparse fp32 rows, add
 * them with their ids as keys, search a small batch, print keys and scores and check every returned score (and the best one of
 * every query) against a merge-join loop in this file.
 *   gcc -std=c99 -Iinclude -o sparse_search examples/sparse_search.c -Lzvec_amd -lzvec_hip -Wl,-rpath,$PWD/zvec_amd
 * Needs an MI355X at run time (there is no CPU fallback: zvec_hip_sparse_create fails without a HIP device). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "zvec_hip.h"

enum { N = 1000, NQ = 3, K = 5, VOCAB = 300, MAXLEN = 24 };

static uint32_t next_word(uint64_t *state) {          /* splitmix64, upper half */
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

/* a run of `count` strictly ascending indices below VOCAB with values in [-1, 1) */
static void make_run(uint64_t *state, uint32_t count, uint32_t *idx, float *val) {
  uint32_t at = next_word(state) % 8;
  for (uint32_t e = 0; e < count; ++e) {
    idx[e] = at;
    val[e] = (float)(next_word(state) % 2000) / 1000.0f - 1.0f;
    at += 1 + next_word(state) % (VOCAB / MAXLEN - 1);
  }
}

/* MINUS the inner product over shared indices, as the reference's merge join computes it; *a = sum of the |products| */
static double score(uint32_t na, const uint32_t *ia, const float *va, uint32_t nb, const uint32_t *ib, const float *vb, double *a) {
  double s = 0.0;
  uint32_t x = 0, y = 0;
  *a = 0.0;
  while (x < na && y < nb) {
    if (ia[x] == ib[y]) {
      s += (double)va[x] * vb[y];
      *a += fabs((double)va[x] * vb[y]);
      ++x;
      ++y;
    } else if (ia[x] < ib[y]) {
      ++x;
    } else {
      ++y;
    }
  }
  return -s;
}

int main(void) {
  zvec_hip_sparse_t index = NULL;
  int rc = zvec_hip_sparse_create(0, &index);
  if (rc != 0) {
    fprintf(stderr, "zvec_hip_sparse_create: %d (%s)\n", rc, zvec_hip_error_string(rc));
    return 1;
  }
  uint32_t *counts = (uint32_t *)malloc(sizeof(uint32_t) * N), *offs = (uint32_t *)malloc(sizeof(uint32_t) * (N + 1));
  uint32_t *idx = (uint32_t *)malloc(sizeof(uint32_t) * N * MAXLEN);
  float *val = (float *)malloc(sizeof(float) * N * MAXLEN);
  uint64_t *ids = (uint64_t *)malloc(sizeof(uint64_t) * N);
  uint64_t state = 11;
  offs[0] = 0;
  for (uint32_t i = 0; i < N; ++i) {
    counts[i] = next_word(&state) % (MAXLEN + 1);        /* empty rows are legal */
    make_run(&state, counts[i], idx + offs[i], val + offs[i]);
    offs[i + 1] = offs[i] + counts[i];
    ids[i] = 5000 + i;
  }
  /* two calls of unequal size */
  if ((rc = zvec_hip_sparse_append(index, counts, idx, val, 300, ids)) != 0) return 2;
  if ((rc = zvec_hip_sparse_append(index, counts + 300, idx + offs[300], val + offs[300], N - 300, ids + 300)) != 0) return 2;
  uint32_t qcounts[NQ] = {MAXLEN, 0, 7}, qoffs[NQ + 1], qidx[NQ * MAXLEN];
  float qval[NQ * MAXLEN];
  qoffs[0] = 0;
  for (int q = 0; q < NQ; ++q) {
    make_run(&state, qcounts[q], qidx + qoffs[q], qval + qoffs[q]);
    qoffs[q + 1] = qoffs[q] + qcounts[q];
  }
  uint64_t keys[NQ * K];
  float scores[NQ * K];
  uint32_t found[NQ];
  rc = zvec_hip_sparse_search(index, NULL, qcounts, qidx, qval, NQ, K, 3.4e38f, NULL, keys, scores, found);
  if (rc != 0) return 3;
  int bad = 0;
  for (int q = 0; q < NQ; ++q) {
    double best = 1e30, a;
    for (uint32_t i = 0; i < N; ++i) {
      const double s = score(counts[i], idx + offs[i], val + offs[i], qcounts[q], qidx + qoffs[q], qval + qoffs[q], &a);
      if (s < best) best = s;
    }
    printf("query %d:", q);
    if (found[q] != K) bad = 1;
    for (uint32_t j = 0; j < found[q]; ++j) {
      const uint64_t key = keys[q * K + j];
      printf(" (%llu, %.6f)", (unsigned long long)key, scores[q * K + j]);
      if (key < 5000 || key >= 5000 + N) { bad = 1; continue; }
      const uint32_t i = (uint32_t)(key - 5000);
      const double s = score(counts[i], idx + offs[i], val + offs[i], qcounts[q], qidx + qoffs[q], qval + qoffs[q], &a);
      /* an fp32 sum of at most MAXLEN products: (MAXLEN + 1) * 2^-23 * sum of the |products| */
      if (fabs(scores[q * K + j] - s) > (MAXLEN + 1) * 1.1920929e-7 * a) bad = 1;
      if (j > 0 && scores[q * K + j] < scores[q * K + j - 1]) bad = 1;
    }
    printf("\n");
    if (found[q] == 0 || fabs(scores[q * K] - best) > (MAXLEN + 1) * 1.1920929e-7 * MAXLEN) bad = 1;
  }
  free(counts); free(offs); free(idx); free(val); free(ids);
  zvec_hip_sparse_destroy(index);
  return bad ? 4 : 0;
}
