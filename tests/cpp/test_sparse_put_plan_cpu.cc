// The host's share of a sparse put (zvec_amd/csrc/host/sparse_put_plan.h: put_keep, put_plan, put_holes, SparsePutLayout) against a
// model of FlatSparseStreamerEntity::add_vector_with_id that takes one row at a time in call order: a row at the count is appended, a
// row behind it pads the gap with holes first, a row below it overwrites (and a written hole stops being one).  After every call the
// kept rows and their order, m, new_n, new_elems, route, gap, the tables (tid, src, sb, tval as SparsePutOffsetsArgs defines it) and
// the hole bits are what the model says.
// Plain host C++, no GPU and no library: g++ -std=c++17 tests/cpp/test_sparse_put_plan_cpu.cc && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zvec_amd/csrc/host/sparse_put_plan.h"

namespace {

constexpr uint32_t MAX_COUNT = 4096, CHUNK = 4096;
int calls = 0;
int routes[3] = {0, 0, 0}, last_route = -1;

#define REQUIRE(cond)                                                                       \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      fprintf(stderr, "call %d: %s failed (%s:%d)\n", calls, #cond, __FILE__, __LINE__);    \
      exit(1);                                                                              \
    }                                                                                       \
  } while (0)

struct Row {
  uint32_t len;
  bool hole;
  int by;        // the row of the current call that wrote it last, -1: none
};

struct Store {
  std::vector<Row> rows;
  HoleWords holes;         // the words under test, carried from call to call
  uint64_t elems() const {
    uint64_t e = 0;
    for (const Row &r : rows) e += r.len;
    return e;
  }
};

// one call on the model and through keep + plan + holes; both must agree
void put(Store &st, const std::vector<uint32_t> &ids, const std::vector<uint32_t> &counts) {
  ++calls;
  const uint64_t n = ids.size(), old_n = st.rows.size(), old_elems = st.elems();
  std::vector<uint64_t> old_off(old_n + 1, 0);
  for (uint64_t r = 0; r < old_n; ++r) old_off[r + 1] = old_off[r] + st.rows[r].len;
  std::vector<uint32_t> old_len(n);                                  // what sparse_put_lens_kernel gives
  for (uint64_t i = 0; i < n; ++i) old_len[i] = ids[i] < old_n ? st.rows[ids[i]].len : 0u;
  const std::vector<Row> before = st.rows;

  // the model, a row at a time
  for (Row &r : st.rows) r.by = -1;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t id = ids[i];
    while (st.rows.size() < id) st.rows.push_back(Row{0, true, -1});
    if (id == st.rows.size()) st.rows.push_back(Row{counts[i], false, (int)i});
    else st.rows[id] = Row{counts[i], false, (int)i};
  }
  const uint64_t new_n = st.rows.size();
  std::vector<uint64_t> new_off(new_n + 1, 0);
  for (uint64_t r = 0; r < new_n; ++r) new_off[r + 1] = new_off[r] + st.rows[r].len;
  std::vector<uint32_t> want_keep;                                   // ascending by position: ascending by id
  uint64_t want_gap = 0, want_m = 0;
  bool want_same = true;
  for (uint64_t r = 0; r < new_n; ++r) {
    if (st.rows[r].by >= 0) {
      want_keep.push_back((uint32_t)st.rows[r].by);
      if (r < old_n) { ++want_m; want_same = want_same && st.rows[r].len == before[r].len; }
    } else if (r >= old_n) {
      REQUIRE(st.rows[r].hole);
      ++want_gap;
    }
  }

  // the code under test
  std::vector<uint32_t> keep;
  REQUIRE(put_keep(ids.data(), n, keep) == 0);
  REQUIRE(keep == want_keep);
  const uint32_t T = (uint32_t)keep.size();
  SparsePutLayout L(T);
  std::vector<uint64_t> ws((size_t)L.tkey + 2, 0xa5a5a5a5a5a5a5a5ull);      // two guard words behind the tables
  SparsePutPlan p;
  REQUIRE(put_plan(p, keep, ids.data(), counts.data(), want_m ? old_len.data() : nullptr, old_n, old_elems, MAX_COUNT, CHUNK, L, ws.data()) == 0);
  REQUIRE(ws[L.tkey] == 0xa5a5a5a5a5a5a5a5ull && ws[L.tkey + 1] == 0xa5a5a5a5a5a5a5a5ull);
  REQUIRE(p.T == T && p.m == want_m && p.old_n == old_n && p.old_elems == old_elems);
  REQUIRE(p.new_n == new_n && p.new_elems == new_off[new_n]);
  REQUIRE(p.same == want_same);
  REQUIRE(p.route == (want_m == 0 ? 0 : want_same ? 1 : 2));
  REQUIRE(p.gap == want_gap);
  REQUIRE(p.tail_base == new_off[old_n]);                            // where the old rows' pairs end afterwards
  ++routes[p.route];
  last_route = p.route;
  const uint32_t *tid = reinterpret_cast<const uint32_t *>(ws.data() + L.tid), *src = reinterpret_cast<const uint32_t *>(ws.data() + L.src);
  const int64_t *tval = reinterpret_cast<const int64_t *>(ws.data() + L.tval);
  const uint64_t *sb = ws.data() + L.sb;
  uint64_t stage = 0;
  int64_t shift = 0;
  for (uint32_t j = 0; j < T; ++j) {
    REQUIRE(tid[j] == ids[keep[j]] && src[j] == keep[j]);
    REQUIRE(j == 0 || tid[j] > tid[j - 1]);
    REQUIRE(sb[j] == stage);
    stage += counts[keep[j]];
    if (j < p.m) {
      // an overwritten row: the new minus the old pairs of the overwritten rows up to and including it, which is what every old
      // offset from this row's end to the next overwritten row's begin moves by
      shift += (int64_t)counts[keep[j]] - (int64_t)before[tid[j]].len;
      REQUIRE(tval[j] == shift);
      REQUIRE((int64_t)new_off[tid[j] + 1] == (int64_t)old_off[tid[j] + 1] + tval[j]);
    } else {
      REQUIRE(tval[j] == (int64_t)new_off[(uint64_t)tid[j] + 1]);    // a tail row: the offset its pairs end at
    }
  }
  REQUIRE(sb[T] == stage && p.S == stage && p.S_over == sb[p.m]);

  // the workspace: every part on a 16-byte boundary, in order, each with room for what it holds
  L.place(p.m, p.S, 2);
  const uint64_t w2 = L.words;
  L.place(p.m, p.S, 4);
  REQUIRE(w2 <= L.words && L.words - w2 <= (p.S * 2 + 7) / 8 + 1);
  const uint64_t part[] = {L.tid, L.src, L.tval, L.sb, L.tkey, L.tbeg, L.ds, L.ss, L.sidx, L.sval, L.words};
  const uint64_t need[] = {((uint64_t)T + 1) / 2, ((uint64_t)T + 1) / 2, T, (uint64_t)T + 1, T, p.m, 2ull * p.m + 3, 2ull * p.m + 2,
                           (p.S + 1) / 2, (p.S * 4 + 7) / 8};
  for (int k = 0; k < 10; ++k) REQUIRE(part[k] % 2 == 0 && part[k] + need[k] <= part[k + 1]);

  // the hole bits: reserved for the new rows first, as SparseWrite::cover does
  st.holes.resize(new_n);
  put_holes(st.holes, p, tid);
  uint64_t holes = 0;
  for (uint64_t r = 0; r < new_n; ++r) {
    REQUIRE(st.holes.is_hole(r) == st.rows[r].hole);
    holes += st.rows[r].hole;
  }
  REQUIRE(st.holes.nholes == holes);
}

Store store_of(const std::vector<uint32_t> &lens) {
  Store st;
  if (lens.empty()) return st;
  std::vector<uint32_t> ids(lens.size());
  for (size_t i = 0; i < lens.size(); ++i) ids[i] = (uint32_t)i;
  put(st, ids, lens);
  return st;
}

}  // namespace

int main() {
  // ---- fixed cases ----
  {
    Store st;                                                        // an empty store: the first row, then a gap in front of a row
    put(st, {0}, {3});
    put(st, {4}, {2});
    put(st, {2, 1}, {0, 5});                                         // two holes written, out of order, one by an empty row
    put(st, {3}, {0});                                               // the last hole by an empty row: in place
    REQUIRE(st.holes.nholes == 0);
  }
  {
    Store st;
    put(st, {3}, {4});                                               // a gap in front of the very first row
    REQUIRE(st.holes.nholes == 3);
    put(st, {4, 9, 10, 70, 200}, {2, 0, 5, 7, 1});                   // gaps that cross 64-bit words of the hole bits
    REQUIRE(st.holes.nholes == 3 + 4 + 59 + 129);
    put(st, {64, 63, 128, 0}, {1, 1, 1, 1});
  }
  const std::vector<uint32_t> base = {5, 9, 0, 7, 12, 3, 30, 1};
  {
    Store st = store_of(base);                                       // ids out of order and twice, a tail row behind a gap
    put(st, {6, 2, 6, 9, 2}, {4, 0, 30, 2, 0});                      // the kept rows keep their lengths: in place
    REQUIRE(last_route == 1);
    put(st, {6, 2, 6, 9, 2}, {30, 1, 29, 2, 3});                     // they do not: splice; the hole at 8 stays, 9 is overwritten now
    REQUIRE(last_route == 2 && st.holes.nholes == 1);
    put(st, {6, 6, 6}, {1, 2, 29});                                  // an id three times, the last as long as the stored row
    REQUIRE(last_route == 1);
  }
  {
    Store st = store_of(base);
    put(st, {0, 7}, {0, 0});                                         // first and last row to empty
    put(st, {0, 7}, {2, 2});                                         // ... and back
    put(st, {7, 8}, {2, 4});                                         // the last row and the next id
    put(st, {9, 10, 11}, {0, 0, 0});                                 // empty rows at the tail are rows, not holes
    REQUIRE(st.holes.nholes == 0);
    put(st, {14, 12}, {1, 1});                                       // tail rows out of order with a gap between and behind
    REQUIRE(st.holes.nholes == 1);
    put(st, {13, 3, 15, 3, 13}, {2, 7, 0, 6, 3});                    // a hole written twice, a row twice, one appended
    put(st, {1, 3, 4}, {4096, 0, 1});                                // the longest row there is
    put(st, {1}, {4096});
  }
  // ---- the refusals ----
  {
    std::vector<uint32_t> keep;
    const uint32_t bad[] = {1, 0xffffffffu, 2}, far[] = {0xfffffffeu}, last[] = {0xfffffffdu}, one[] = {6};
    REQUIRE(put_keep(bad, 3, keep) == ZVEC_HIP_ERR_OUT_OF_RANGE);    // kInvalidNodeId
    REQUIRE(put_keep(bad, 1, keep) == 0 && keep.size() == 1);
    SparsePutLayout L(1);
    std::vector<uint64_t> ws((size_t)L.tkey, 0);
    SparsePutPlan p;
    REQUIRE(put_keep(far, 1, keep) == 0);
    REQUIRE(put_plan(p, keep, far, one, nullptr, 8, 100, MAX_COUNT, CHUNK, L, ws.data()) == ZVEC_HIP_ERR_OUT_OF_RANGE);      // 2^32 - 1 rows
    REQUIRE(put_plan(p, keep, last, one, nullptr, 8, 100, MAX_COUNT, CHUNK, L, ws.data()) == 0 && p.new_n == 0xfffffffeull && p.route == 0);
    REQUIRE(p.gap == 0xfffffffeull - 8 - 1);
    // an old length no store has; and a splice whose grid does not fit (the same call in place is taken)
    const uint32_t id2[] = {2}, too_long[] = {MAX_COUNT + 1}, five[] = {5};
    REQUIRE(put_plan(p, keep, id2, one, too_long, 8, 100, MAX_COUNT, CHUNK, L, ws.data()) == ZVEC_HIP_ERR_RUNTIME);
    const uint64_t huge = 0x7fffffffull * CHUNK;
    REQUIRE(put_plan(p, keep, id2, one, five, 8, huge, MAX_COUNT, CHUNK, L, ws.data()) == ZVEC_HIP_ERR_OUT_OF_RANGE);
    REQUIRE(put_plan(p, keep, id2, five, five, 8, huge, MAX_COUNT, CHUNK, L, ws.data()) == 0 && p.route == 1);
    REQUIRE(put_plan(p, keep, id2, one, five, 8, huge - 1, MAX_COUNT, CHUNK, L, ws.data()) == 0 && p.route == 2 && p.new_elems == huge);
  }
  // ---- pseudo-random calls (fixed seed) on stores of at most 12 rows ----
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  Store st;
  for (int i = 0; i < 4000; ++i) {
    if (st.rows.size() >= 12 || rnd() % 16 == 0) {
      std::vector<uint32_t> lens(rnd() % 9);
      for (uint32_t &l : lens) l = (uint32_t)(rnd() % 6);
      st = store_of(lens);
    }
    const uint64_t cnt = st.rows.size(), n = 1 + rnd() % 8;
    const bool keep_lengths = rnd() % 2 == 0, ascending = rnd() % 4 == 0;
    std::vector<uint32_t> ids(n);
    for (uint64_t r = 0; r < n; ++r) {
      const uint64_t kind = rnd() % 8;                               // below, at and behind the count; a repeat of an earlier row's id
      if (r && kind == 0) ids[r] = ids[rnd() % r];
      else if (kind < 4 && cnt) ids[r] = (uint32_t)(rnd() % cnt);
      else ids[r] = (uint32_t)(cnt + rnd() % 4);
    }
    if (ascending) {                                                 // (the route that skips the sort)
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    std::vector<uint32_t> counts(ids.size());
    for (size_t r = 0; r < ids.size(); ++r) counts[r] = keep_lengths && ids[r] < cnt ? st.rows[ids[r]].len : (uint32_t)(rnd() % 6);
    put(st, ids, counts);
  }
  REQUIRE(routes[0] > 300 && routes[1] > 300 && routes[2] > 300);
  printf("sparse put plan: %d calls (tail %d, in place %d, splice %d)\nok\n", calls, routes[0], routes[1], routes[2]);
  return 0;
}
