/* examples/sparse_put.c — add-with-id on a sparse index from plain C: documents go in one by one under their ids, as zvec's
 * Index::_sparse_add does; two ids are left out (the gap is padded with holes), one document is then replaced by a longer one
 * (the rows behind it move on the device), one query is searched and its list is checked against a merge-join loop in this file
 * over the documents as they stand after the replacement.
 *   gcc -std=c99 -Iinclude -o sparse_put examples/sparse_put.c -Lzvec_amd -lzvec_hip -lm -Wl,-rpath,$PWD/zvec_amd
 * Needs an MI355X at run time (there is no CPU fallback: zvec_hip_sparse_create fails without a HIP device). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "zvec_hip.h"

enum { N = 200, K = 8, MAXLEN = 16, LONGLEN = 40, STEP = 7, GAP0 = 50, GAP1 = 51, REPLACED = 20 };

static uint32_t next_word(uint64_t *state) {          /* splitmix64, upper half */
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

/* a run of `count` strictly ascending indices with values in [-1, 1) */
static void make_run(uint64_t *state, uint32_t count, uint32_t *idx, float *val) {
  uint32_t at = next_word(state) % 4;
  for (uint32_t e = 0; e < count; ++e) {
    idx[e] = at;
    val[e] = (float)(next_word(state) % 2000) / 1000.0f - 1.0f;
    at += 1 + next_word(state) % STEP;
  }
}

/* MINUS the inner product over shared indices; *a = sum of the |products| */
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
  static uint32_t counts[N], idx[N][LONGLEN];
  static float val[N][LONGLEN];
  zvec_hip_sparse_t index = NULL;
  int rc = zvec_hip_sparse_create(0, &index);
  if (rc != 0) {
    fprintf(stderr, "zvec_hip_sparse_create: %d (%s)\n", rc, zvec_hip_error_string(rc));
    return 1;
  }
  uint64_t state = 23;
  memset(counts, 0, sizeof(counts));
  for (uint32_t id = 0; id < N; ++id) {
    if (id == GAP0 || id == GAP1) continue;              /* never added: positions 50 and 51 become holes */
    counts[id] = 1 + next_word(&state) % MAXLEN;
    make_run(&state, counts[id], idx[id], val[id]);
    if ((rc = zvec_hip_sparse_put(index, &id, &counts[id], idx[id], val[id], 1, NULL)) != 0) return 2;
  }
  /* document 20 again, longer: everything stored behind it moves */
  uint32_t id = REPLACED;
  counts[id] = LONGLEN;
  make_run(&state, counts[id], idx[id], val[id]);
  if ((rc = zvec_hip_sparse_put(index, &id, &counts[id], idx[id], val[id], 1, NULL)) != 0) return 2;
  int route = -1;
  uint64_t rows = 0, pairs = 0, holes = 0, want_pairs = 0;
  for (uint32_t i = 0; i < N; ++i) want_pairs += counts[i];
  if (zvec_hip_sparse_put_info(index, &route, NULL, NULL, NULL) != 0 || zvec_hip_sparse_count(index, &rows, &pairs) != 0 ||
      zvec_hip_sparse_holes(index, &holes) != 0)
    return 3;
  printf("rows %llu, pairs %llu, holes %llu, route of the last put %d\n", (unsigned long long)rows, (unsigned long long)pairs,
         (unsigned long long)holes, route);
  int bad = rows != N || pairs != want_pairs || holes != 2 || route != 2;

  uint32_t qcount = MAXLEN, qidx[MAXLEN];
  float qval[MAXLEN];
  make_run(&state, qcount, qidx, qval);
  uint64_t keys[K];
  float scores[K];
  uint32_t found = 0;
  if ((rc = zvec_hip_sparse_search(index, NULL, &qcount, qidx, qval, 1, K, 3.4e38f, NULL, keys, scores, &found)) != 0) return 4;
  double best = 1e30, a;
  for (uint32_t i = 0; i < N; ++i) {
    if (i == GAP0 || i == GAP1) continue;
    const double s = score(counts[i], idx[i], val[i], qcount, qidx, qval, &a);
    if (s < best) best = s;
  }
  printf("query:");
  if (found != K) bad = 1;
  for (uint32_t j = 0; j < found; ++j) {
    printf(" (%llu, %.6f)", (unsigned long long)keys[j], scores[j]);
    if (keys[j] >= N || keys[j] == GAP0 || keys[j] == GAP1) { bad = 1; continue; }     /* a hole is never returned */
    const uint32_t i = (uint32_t)keys[j];
    const double s = score(counts[i], idx[i], val[i], qcount, qidx, qval, &a);
    /* an fp32 sum of at most MAXLEN products: (MAXLEN + 1) * 2^-23 * sum of the |products| */
    if (fabs(scores[j] - s) > (MAXLEN + 1) * 1.1920929e-7 * a) bad = 1;
    if (j > 0 && scores[j] < scores[j - 1]) bad = 1;
  }
  printf("\n");
  if (found == 0 || fabs(scores[0] - best) > (MAXLEN + 1) * 1.1920929e-7 * MAXLEN) bad = 1;
  printf("check %s\n", bad ? "FAILED" : "passed");
  zvec_hip_sparse_destroy(index);
  return bad ? 5 : 0;
}
