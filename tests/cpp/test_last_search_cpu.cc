// zvec_amd/csrc/host/last_search.h without a GPU: the record a context keeps of its last user-facing search.  Beginning a search of
// any family leaves nothing of another family readable; the readers' admission rule over family, owner and count; a pending certify
// step goes with any begin; and the two ways a search nests — passes that only OR into the route word, and the certify step that takes
// its numbers before the searches it re-runs begin the record anew.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../zvec_amd/csrc/host/last_search.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      exit(1);                                                    \
    }                                                             \
  } while (0)

typedef LastSearch::Family Family;
static const Family FAMILIES[] = {LastSearch::FLAT, LastSearch::IVF, LastSearch::HAMMING_IVF, LastSearch::HNSW, LastSearch::SPARSE};
static const int A = 0, B = 0;             // two handles: only their addresses matter

// a finished search of family f on handle h with n queries, every mark a family could leave set to something
static void search(LastSearch &r, Family f, const void *h, uint32_t n) {
  r.begin(f, h);
  r.route = 0x123;
  r.ivf.route = ZVEC_HIP_IVF_ROUTE_TILE; r.ivf.nq = n; r.ivf.words = 64; r.ivf.o_qscanned = 4;
  r.bivf_np = 3; r.bivf_cand_kc = 8; r.bivf_cand_slice = 2;
  r.hnsw_slices = 5;
  r.certify.count = n; r.certify.kp = 32; r.certify.topk = 10;
  r.count = n;
}

// nothing but the family and the owner of the search just begun is left
static void check_begun(const LastSearch &r, Family f, const void *h) {
  CHECK(r.family == f && r.owner == h && r.count == 0);
  CHECK(r.route == 0 && r.flat_route() == 0);
  CHECK(r.ivf.route == ZVEC_HIP_IVF_ROUTE_NONE && r.ivf.words == 0 && r.ivf.o_qscanned == 0 && !r.ivf.has_stats());
  CHECK(r.ivf_plan().route == ZVEC_HIP_IVF_ROUTE_NONE);
  CHECK(r.bivf_np == 0 && r.bivf_cand_kc == 0 && r.bivf_cand_slice == 0 && r.hnsw_slices == 0);
  CHECK(r.certify.count == 0 && r.certify.kp == 0 && r.certify.topk == 0);
  for (Family g : FAMILIES)
    for (uint32_t n : {0u, 1u, 4u}) CHECK(!r.admits(g, h, n));
}

int main() {
  // the empty record admits nobody and reports nothing
  {
    LastSearch r;
    check_begun(r, LastSearch::NONE, nullptr);
    CHECK(!r.admits(LastSearch::NONE, nullptr, 0));
    CHECK(r.take_certify().count == 0);
  }
  // every ordered pair of families, the same family on another handle included: a begin wipes all of it
  for (Family f : FAMILIES)
    for (Family g : FAMILIES) {
      LastSearch r;
      search(r, f, &A, 4);
      r.begin(g, f == g ? (const void *)&B : (const void *)&A);
      check_begun(r, g, f == g ? (const void *)&B : (const void *)&A);
    }
  // ... and so does the writers' form of it
  {
    LastSearch r;
    search(r, LastSearch::HNSW, &A, 4);
    r.begin(LastSearch::NONE, nullptr);
    check_begun(r, LastSearch::NONE, nullptr);
  }
  // the admission rule: family, owner, count, count + 1
  for (Family f : FAMILIES) {
    LastSearch r;
    search(r, f, &A, 4);
    CHECK(r.admits(f, &A, 4) && r.admits(f, &A, 1) && r.admits(f, &A, 0));
    CHECK(!r.admits(f, &A, 5));
    CHECK(!r.admits(f, &B, 4) && !r.admits(f, nullptr, 4));
    for (Family g : FAMILIES)
      if (g != f) CHECK(!r.admits(g, &A, 4));
    CHECK(!r.admits(LastSearch::NONE, &A, 4));
    // the readers that take no handle follow the family alone
    CHECK(r.flat_route() == (f == LastSearch::FLAT ? 0x123u : 0u));
    CHECK(r.ivf_plan().route == (f == LastSearch::IVF ? ZVEC_HIP_IVF_ROUTE_TILE : ZVEC_HIP_IVF_ROUTE_NONE));
    CHECK(r.ivf_plan().words == (f == LastSearch::IVF ? 64u : 0u));
    // a search that has not set its count yet (or failed half-way) admits nobody
    r.begin(f, &A);
    r.hnsw_slices = 1;
    CHECK(!r.admits(f, &A, 0) && !r.admits(f, &A, 1));
  }
  // which IVF routes leave per-query numbers
  {
    IvfPlanMark m;
    CHECK(!m.has_stats());
    for (uint32_t route : {ZVEC_HIP_IVF_ROUTE_DIRECT_BLOCK_TOPK, ZVEC_HIP_IVF_ROUTE_DIRECT_SELECT, ZVEC_HIP_IVF_ROUTE_TILE}) {
      m.route = route;
      CHECK(m.has_stats());
    }
    m.route = ZVEC_HIP_IVF_ROUTE_LARGE_K;
    CHECK(!m.has_stats());
  }
  // a pending certify step is dropped by beginning any search
  for (Family g : FAMILIES) {
    LastSearch r;
    r.begin(LastSearch::FLAT, &A);
    r.count = 4; r.certify.count = 4; r.certify.kp = 32; r.certify.topk = 10;
    r.begin(g, &A);
    CHECK(r.certify.count == 0 && r.take_certify().count == 0);
  }
  // nesting, first form: a pass inside a search of another family (the IVF coarse pass through the flat scan) only ORs into the
  // route word; the outer search's marks stay and the word cannot be read
  {
    LastSearch r;
    r.begin(LastSearch::IVF, &A);
    r.route |= 0x22;
    r.ivf.route = ZVEC_HIP_IVF_ROUTE_DIRECT_SELECT; r.ivf.nq = 2; r.ivf.o_qscanned = 2;
    r.count = 2;
    CHECK(r.flat_route() == 0);
    CHECK(r.admits(LastSearch::IVF, &A, 2) && r.ivf_plan().route == ZVEC_HIP_IVF_ROUTE_DIRECT_SELECT && r.ivf.o_qscanned == 2);
    CHECK(!r.admits(LastSearch::FLAT, &A, 1));
    // ... and inside a flat search (the seeding prefix's own scan) the outer word is put aside and folded back by the scan itself
    r.begin(LastSearch::FLAT, &A);
    r.route |= 0x400;
    const uint32_t outer = r.route;
    r.route = 0;
    r.route |= 0x2;                        // the prefix's scan
    r.route = outer | ((r.route & 0x3ffu) << 16);
    r.route |= 0x20;
    CHECK(r.flat_route() == (0x400u | (0x2u << 16) | 0x20u) && r.family == LastSearch::FLAT && r.owner == &A);
  }
  // nesting, second form: the certify step takes its numbers, then the searches it re-runs begin the record anew; what it took is its
  // own, and the step the re-run leaves is the re-run's
  {
    LastSearch r;
    r.begin(LastSearch::IVF, &A);
    r.count = 8; r.certify.count = 8; r.certify.kp = 24; r.certify.topk = 10;
    CHECK(r.admits(LastSearch::IVF, &A, 8) && r.certify.count == 8);
    const LastSearch::Certify step = r.take_certify();
    CHECK(step.count == 8 && step.kp == 24 && step.topk == 10);
    CHECK(r.certify.count == 0 && r.certify.kp == 0 && r.certify.topk == 0);
    CHECK(r.admits(LastSearch::IVF, &A, 8));             // (taking the step leaves the rest of the record)
    r.begin(LastSearch::IVF, &A);                        // the second pass over 3 flagged queries, twice as wide
    r.count = 3; r.certify.count = 3; r.certify.kp = 48; r.certify.topk = 10;
    CHECK(step.count == 8 && step.kp == 24);
    CHECK(r.admits(LastSearch::IVF, &A, 3) && !r.admits(LastSearch::IVF, &A, 8));
    const LastSearch::Certify inner = r.take_certify();
    CHECK(inner.count == 3 && inner.kp == 48 && r.certify.count == 0);
  }
  printf("ok\n");
  return 0;
}
