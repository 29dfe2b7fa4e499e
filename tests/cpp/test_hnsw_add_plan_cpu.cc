// test_hnsw_add_plan_cpu.cc — zvec_amd/csrc/host/hnsw_add_plan.h without a GPU and without HIP: the rounds from a base against a
// restatement, the request offsets of the new nodes, the levels of a range, the capacity steps, the stride decision, the refusals,
// a few thousand random call sequences in which the plan of a graph grown call by call is held to DESIGN §3c "Appending", and the
// one plan of both entries (hnsw_insert_plan) against the composition of the small functions, in those sequences and in fixed cases.
// Built by tests/test_hnsw_add_plan_cpu.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../zvec_amd/csrc/host/hnsw_add_plan.h"

#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #c);      \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

namespace {

// DESIGN §3c "Rounds", written again: one round at a time from s, over the levels of ALL nodes
struct Step { uint32_t first, end, entry, top; };
std::vector<Step> restated(const std::vector<uint32_t> &lv, uint32_t base, uint32_t end, uint32_t div, uint32_t mx, uint32_t &entry, uint32_t &top) {
  std::vector<Step> out;
  uint32_t s = base;
  if (base == 0) { entry = 0; top = end ? lv[0] : 0; s = 1; }
  while (s < end) {
    uint32_t size = div == 0 ? 1 : s / div;
    if (size < 1) size = 1;
    if (size > mx) size = mx;
    uint32_t e = s + 1;
    if (lv[s] <= top)
      while (e < end && e < s + size && lv[e] <= top) ++e;
    out.push_back({s, e, entry, top});
    if (lv[s] > top) { entry = s; top = lv[s]; }
    s = e;
  }
  return out;
}

void check_call(const std::vector<uint32_t> &lv, uint32_t base, uint32_t count, uint32_t div, uint32_t mx, uint32_t m0, uint32_t m, uint32_t &entry,
                uint32_t &top) {
  uint32_t e2 = entry, t2 = top;
  std::vector<HnswRound> plan;
  std::vector<uint64_t> off;
  hnsw_plan_rounds(base, lv.data() + base, count, div, mx, m0, m, entry, top, plan, off);
  const std::vector<Step> want = restated(lv, base, base + count, div, mx, e2, t2);
  EXPECT(plan.size() == want.size() && entry == e2 && top == t2);
  EXPECT(off.size() == (size_t)count + 1 && off[0] == 0);
  uint32_t next = base == 0 ? 1 : base;
  for (size_t r = 0; r < plan.size(); ++r) {
    EXPECT(plan[r].first == want[r].first && plan[r].end == want[r].end && plan[r].entry == want[r].entry && plan[r].top == want[r].top);
    EXPECT(plan[r].first == next && plan[r].end > plan[r].first && plan[r].end <= base + count);      // contiguous, inside the call
    next = plan[r].end;
    for (uint32_t i = plan[r].first; i < plan[r].end; ++i) {
      const uint32_t searched = std::min(lv[i], plan[r].top);
      EXPECT(off[i - base + 1] - off[i - base] == m0 + (uint64_t)searched * m);
      EXPECT(i == plan[r].first || lv[i] <= plan[r].top);                                              // a raiser is alone and first
    }
    if (lv[plan[r].first] > plan[r].top) EXPECT(plan[r].end == plan[r].first + 1);
  }
  EXPECT(count == 0 || next == base + count || (base == 0 && count == 1));
  if (base == 0 && count) EXPECT(off[1] == 0);                                                         // the seed asks for nothing
}

bool same_shape(const HnswShape &a, const HnswShape &b) {
  return a.n == b.n && a.cap_rows == b.cap_rows && a.cap_upper == b.cap_upper && a.m0 == b.m0 && a.m == b.m && a.stride == b.stride &&
         a.n_upper == b.n_upper && a.entry == b.entry;
}
bool same_params(const zvec_hip_hnsw_build_params &a, const zvec_hip_hnsw_build_params &b) {
  return a.m == b.m && a.m0 == b.m0 && a.ef_construction == b.ef_construction && a.prune_cnt == b.prune_cnt &&
         a.min_neighbors == b.min_neighbors && a.scaling_factor == b.scaling_factor && a.seed == b.seed;
}

// hnsw_insert_plan against the small functions composed by hand, as the two entries composed them before there was one plan
void check_plan(const HnswShape &found, const zvec_hip_hnsw_build_params &rem, uint64_t want_rows, uint64_t want_upper, const uint32_t *lv,
                uint32_t count, const zvec_hip_hnsw_build_params *p, uint32_t div, uint32_t mx, uint64_t budget, bool append, HnswInsertPlan &pl) {
  EXPECT(hnsw_insert_plan(found, rem, want_rows, want_upper, count, true, p, lv, div, mx, budget, append, pl) == 0);
  zvec_hip_hnsw_build_params q{};
  EXPECT(hnsw_add_params(p, rem, found.n, found.m0, found.m, q) == 0 && same_params(q, pl.q));
  std::vector<uint32_t> levels;
  EXPECT(hnsw_add_levels(found.n, count, lv, q, levels) == 0 && levels == pl.lv);
  std::vector<HnswRound> rounds;
  std::vector<uint64_t> off;
  uint32_t entry = found.entry, top = found.stride;
  hnsw_plan_rounds((uint32_t)found.n, levels.data(), count, div, mx, q.m0, q.m, entry, top, rounds, off);
  EXPECT(pl.base == found.n && pl.count == count && pl.top == top && pl.after.entry == entry && off == pl.req_off && rounds.size() == pl.rounds.size());
  for (size_t r = 0; r < rounds.size(); ++r)
    EXPECT(rounds[r].first == pl.rounds[r].first && rounds[r].end == pl.rounds[r].end && rounds[r].entry == pl.rounds[r].entry && rounds[r].top == pl.rounds[r].top);
  std::vector<uint32_t> upper_of(count);
  const HnswAddShape sh = hnsw_add_shape(found.stride, found.n_upper, levels.data(), count, upper_of.data());
  EXPECT(upper_of == pl.upper_of && sh.restride == pl.restride && sh.stride == pl.after.stride && sh.n_upper == pl.after.n_upper);
  const HnswRoundsNeed need = hnsw_rounds_need(rounds, off, (uint32_t)found.n, budget);
  EXPECT(need.max_slots == pl.need.max_slots && need.max_ws == pl.need.max_ws && need.multi == pl.need.multi && pl.budget == budget);
  EXPECT(pl.after.n == found.n + count && pl.after.m0 == q.m0 && pl.after.m == (sh.stride ? q.m : 0));
  EXPECT(pl.after.cap_rows == hnsw_grow(found.cap_rows, found.n + count, want_rows));
  EXPECT(pl.after.cap_upper == (sh.stride ? hnsw_grow(found.cap_upper, sh.n_upper, want_upper) : 0));
  EXPECT(same_shape(hnsw_shape_kept(pl.after), pl.after));                             // what a plan leaves needs no tidying
}

void insert_plan_cases() {
  const zvec_hip_hnsw_build_params none{};
  zvec_hip_hnsw_build_params p{};
  p.m = 4; p.m0 = 8; p.ef_construction = 16; p.scaling_factor = 5; p.seed = 77;
  std::vector<uint32_t> lv(600);
  EXPECT(hnsw_levels_range(0, 600, 5, 77, lv.data()) == 0);
  uint32_t n_upper = 0;
  for (uint32_t v : lv) n_upper += v >= 1;
  EXPECT(n_upper > 60 && n_upper < 300);
  const HnswShape empty;
  HnswInsertPlan build, add, gen;
  // a build: empty shape, nothing remembered, nothing wanted; the capacities are exactly (n, n_upper)
  check_plan(empty, none, 0, 0, lv.data(), 600, &p, 16, 64, 1 << 20, false, build);
  EXPECT(build.after.cap_rows == 600 && build.after.cap_upper == n_upper && build.after.n_upper == n_upper && build.restride && build.base == 0);
  // the same rows as an add on an empty handle that a reserve(600, 300) went before
  check_plan(empty, none, 600, 300, lv.data(), 600, &p, 16, 64, 1 << 20, true, add);
  EXPECT(add.after.cap_rows == 600 && add.after.cap_upper == 300 && add.restride && add.rounds.size() == build.rounds.size());
  add.after.cap_upper = n_upper;
  EXPECT(same_shape(add.after, build.after) && add.req_off == build.req_off && add.upper_of == build.upper_of);
  // generated levels are the given ones
  EXPECT(hnsw_insert_plan(empty, none, 0, 0, 600, true, &p, nullptr, 16, 64, 1 << 20, false, gen) == 0 && gen.lv == lv && same_shape(gen.after, build.after));
  // count == 0 on a graph: an empty plan, the shape as found
  HnswShape g = build.after;
  HnswInsertPlan zero;
  zero.count = 9;
  EXPECT(hnsw_insert_plan(g, p, 1000, 1000, 0, false, nullptr, nullptr, 16, 64, 1 << 20, true, zero) == 0);
  EXPECT(zero.rounds.empty() && zero.lv.empty() && zero.count == 0 && same_shape(zero.after, g) && !zero.restride && zero.q.m0 == 8 && zero.q.seed == 77);
  // ... and an add of no rows does not ask whether levels could be generated, a build of no rows does (scaling_factor 4)
  zvec_hip_hnsw_build_params p4 = p;
  p4.scaling_factor = 4;
  EXPECT(hnsw_insert_plan(empty, none, 0, 0, 0, false, &p4, nullptr, 16, 64, 1 << 20, true, zero) == 0);
  EXPECT(hnsw_insert_plan(empty, none, 0, 0, 0, false, &p4, nullptr, 16, 64, 1 << 20, false, zero) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
  EXPECT(hnsw_insert_plan(empty, none, 0, 0, 0, false, &p, nullptr, 16, 64, 1 << 20, false, zero) == 0);       // a build of no rows
  EXPECT(zero.rounds.empty() && zero.after.n == 0 && zero.after.m0 == 8 && zero.after.m == 0 && zero.after.cap_rows == 0 && zero.top == 0);
  // one row on an empty shape: the seed, no round
  check_plan(empty, none, 0, 0, lv.data(), 1, &p, 16, 64, 1 << 20, false, zero);
  EXPECT(zero.rounds.empty() && zero.after.n == 1 && zero.after.cap_rows == 1 && zero.after.entry == 0);
  // a first upper node sets restride, and makes room for the upper table; level-0 rows alone do neither
  HnswShape flat;
  flat.n = flat.cap_rows = 10; flat.m0 = 8;
  const uint32_t first_upper[3] = {0, 2, 0}, level0[3] = {0, 0, 0};
  HnswInsertPlan up;
  check_plan(flat, none, 0, 0, first_upper, 3, &p, 16, 64, 1 << 20, true, up);
  EXPECT(up.restride && up.after.stride == 2 && up.after.n_upper == 1 && up.after.cap_upper == 1 && up.after.m == 4 && up.after.entry == 11 && up.top == 2);
  EXPECT(up.after.cap_rows == 20);
  check_plan(flat, none, 0, 0, level0, 3, &p, 16, 64, 1 << 20, true, up);
  EXPECT(!up.restride && up.after.stride == 0 && up.after.cap_upper == 0 && up.after.m == 0);

  // refusals: the codes of hnsw_add_params and hnsw_add_levels come back as they are, and a refused plan leaves its output alone
  HnswInsertPlan keep = build;
  auto refused = [&](int rc, int want) {
    EXPECT(rc == want);
    EXPECT(same_shape(keep.after, build.after) && same_params(keep.q, build.q) && keep.lv == build.lv && keep.rounds.size() == build.rounds.size() &&
           keep.req_off == build.req_off && keep.upper_of == build.upper_of && keep.count == build.count && keep.top == build.top);
  };
  auto plan = [&](const HnswShape &found, uint64_t count, bool have_rows, const zvec_hip_hnsw_build_params &pp, const uint32_t *levels, bool append,
                  uint32_t mx = 64) { return hnsw_insert_plan(found, none, 0, 0, count, have_rows, &pp, levels, 16, mx, 1 << 20, append, keep); };
  zvec_hip_hnsw_build_params bad = p;
  bad.m0 = 16;
  refused(plan(g, 3, true, bad, level0, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);          // m0 disagrees with the graph
  bad = p; bad.m = 8;
  refused(plan(g, 3, true, bad, level0, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);          // m disagrees with the upper lists
  bad = p; bad.ef_construction = 513;
  refused(plan(g, 3, true, bad, level0, true), ZVEC_HIP_ERR_UNSUPPORTED);
  refused(plan(empty, 3, true, bad, level0, false), ZVEC_HIP_ERR_UNSUPPORTED);
  bad = p; bad.m0 = 257;
  refused(plan(empty, 3, true, bad, level0, false), ZVEC_HIP_ERR_UNSUPPORTED);
  bad = p; bad.m = 129;
  refused(plan(empty, 3, true, bad, level0, false), ZVEC_HIP_ERR_UNSUPPORTED);
  bad = p; bad.min_neighbors = 5;
  refused(plan(g, 3, true, bad, level0, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);
  HnswShape no_lists = flat;
  no_lists.m0 = 0;
  refused(plan(no_lists, 3, true, none, level0, true), ZVEC_HIP_ERR_UNSUPPORTED);       // a loaded graph without level-0 lists
  const uint32_t high[3] = {0, 16, 0};
  refused(plan(g, 3, true, p, high, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);              // a level of 16
  refused(plan(empty, 3, true, p, high, false), ZVEC_HIP_ERR_INVALID_ARGUMENT);
  refused(plan(g, 3, true, p4, nullptr, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);          // generated levels want 5 .. 1000
  refused(plan(g, 0xfffffff0ull, true, p, level0, true), ZVEC_HIP_ERR_OUT_OF_RANGE);
  refused(plan(g, ~0ull, true, p, level0, true), ZVEC_HIP_ERR_OUT_OF_RANGE);
  refused(plan(g, 3, false, p, level0, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);           // no rows
  refused(plan(empty, 3, false, p, level0, false), ZVEC_HIP_ERR_INVALID_ARGUMENT);
  // where two faults coincide each entry keeps its order: a build tests the range before the rows, an add the rows before the range;
  // the parameters come first in both
  refused(plan(empty, 0xfffffff0ull, false, p, level0, false), ZVEC_HIP_ERR_OUT_OF_RANGE);
  refused(plan(g, 0xfffffff0ull, false, p, level0, true), ZVEC_HIP_ERR_INVALID_ARGUMENT);
  refused(plan(empty, 0xfffffff0ull, false, bad, level0, false), ZVEC_HIP_ERR_INVALID_ARGUMENT);
  bad = p; bad.ef_construction = 513;
  refused(plan(g, 0, false, bad, nullptr, true), ZVEC_HIP_ERR_UNSUPPORTED);             // an add of no rows still reads its parameters
  // one round of 986896 nodes with 256 + 15 * 128 = 2176 request slots each is 2^31 + 2048 slots, which the sort and the group starts do
  // not count; one node fewer is 2^31 - 128
  zvec_hip_hnsw_build_params wide = none;
  wide.m = 128; wide.m0 = 256; wide.ef_construction = 16;
  HnswShape big;
  big.n = big.cap_rows = 1u << 24; big.m0 = 256; big.m = 128; big.stride = 15; big.n_upper = big.cap_upper = 1;
  std::vector<uint32_t> l15(1u << 20, 15);
  refused(plan(big, 986896, true, wide, l15.data(), true, 1u << 20), ZVEC_HIP_ERR_UNSUPPORTED);
  EXPECT(plan(big, 986895, true, wide, l15.data(), true, 1u << 20) == 0 && keep.need.max_slots == (1ull << 31) - 128 && keep.rounds.size() == 1);
}

void fixed_cases() {
  // the build's plan of 35 level-0 nodes under round_div 16: one node a round up to 32 nodes, then [32, 34) and [34, 35)
  std::vector<uint32_t> lv(35, 0);
  uint32_t entry = 9, top = 9;
  std::vector<HnswRound> plan;
  std::vector<uint64_t> off;
  hnsw_plan_rounds(0, lv.data(), 35, 16, 64, 8, 4, entry, top, plan, off);
  EXPECT(plan.size() == 33 && plan[31].first == 32 && plan[31].end == 34 && plan[32].first == 34 && plan[32].end == 35);
  EXPECT(entry == 0 && top == 0 && off[35] == 34 * 8);
  // the same rows cut at 33: the round [32, 34) ends at the call boundary
  entry = top = 0;
  hnsw_plan_rounds(0, lv.data(), 33, 16, 64, 8, 4, entry, top, plan, off);
  EXPECT(plan.back().first == 32 && plan.back().end == 33);
  hnsw_plan_rounds(33, lv.data() + 33, 2, 16, 64, 8, 4, entry, top, plan, off);
  EXPECT(plan.size() == 1 && plan[0].first == 33 && plan[0].end == 35 && off[2] == 16);
  // a raiser in the middle of a call: rounds [100, 103) [103, 104) [104, 110) [110, 116) [116, 120), the entry point moves after its round
  std::vector<uint32_t> l2(120, 0);
  l2[103] = 2;
  entry = 7; top = 1;
  hnsw_plan_rounds(100, l2.data() + 100, 20, 16, 64, 8, 4, entry, top, plan, off);
  EXPECT(plan.size() == 5 && plan[0].end == 103 && plan[1].first == 103 && plan[1].end == 104 && plan[1].entry == 7 && plan[1].top == 1);
  EXPECT(plan[2].entry == 103 && plan[2].top == 2 && plan[2].first == 104 && plan[2].end == 110 && plan[3].end == 116 && plan[4].end == 120 && entry == 103 && top == 2);
  EXPECT(off[4] - off[3] == 8 + 1 * 4);           // searched on level 1 and 0: min(level, top) = 1
  // round_div 0: every round has one node
  entry = 0; top = 0;
  hnsw_plan_rounds(50, lv.data(), 30, 0, 64, 8, 4, entry, top, plan, off);
  EXPECT(plan.size() == 30);
  const HnswRoundsNeed need = hnsw_rounds_need(plan, off, 50, 1 << 20);
  EXPECT(need.multi == 0 && need.max_slots == 8 && need.max_ws == 4 * 3);
  // slices: 34 nodes at s = 1030 need 4 * 33 + 8 * 1030 bytes each
  EXPECT(hnsw_round_node_bytes(1030) == 8372 && hnsw_round_node_bytes(1024) == 128);
  const HnswRound r{1030, 1064, 0, 0};
  EXPECT(hnsw_round_slice(r, 1ull << 30) == 34 && hnsw_round_slice(r, 103776) == 12 && hnsw_round_slice(r, 17296) == 2 && hnsw_round_slice(r, 1024) == 1);
}

void levels_and_params() {
  // the levels of a range are the levels of the whole, whatever the split
  std::vector<uint32_t> whole(5000), part(5000);
  EXPECT(hnsw_levels_range(0, 5000, 5, 77, whole.data()) == 0);
  EXPECT(hnsw_levels_range(0, 1234, 5, 77, part.data()) == 0 && hnsw_levels_range(1234, 1, 5, 77, part.data() + 1234) == 0 &&
         hnsw_levels_range(1235, 3765, 5, 77, part.data() + 1235) == 0);
  EXPECT(whole == part);
  uint32_t above = 0, top = 0;
  for (uint32_t v : whole) { above += v >= 1; top = std::max(top, v); }
  EXPECT(above > 800 && above < 1200 && top >= 2 && top <= HNSW_PLAN_MAX_LEVEL);      // P(level >= 1) = 1 / 5
  EXPECT(hnsw_levels_range(0, 1, 4, 0, whole.data()) == ZVEC_HIP_ERR_INVALID_ARGUMENT && hnsw_levels_range(0, 1, 1001, 0, whole.data()) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
  EXPECT(hnsw_levels_range(0, 1, 8, 0, nullptr) == ZVEC_HIP_ERR_INVALID_ARGUMENT && hnsw_levels_range(0, 0, 8, 0, nullptr) == 0);

  zvec_hip_hnsw_build_params none{}, q{}, p{}, rem{};
  EXPECT(hnsw_add_params(nullptr, none, 0, 0, 0, q) == 0);                             // the reference's defaults
  EXPECT(q.m == 50 && q.m0 == 100 && q.ef_construction == 500 && q.prune_cnt == 50 && q.scaling_factor == 50 && q.min_neighbors == 0 && q.seed == 0);
  rem.m = 4; rem.m0 = 8; rem.ef_construction = 16; rem.prune_cnt = 3; rem.min_neighbors = 2; rem.scaling_factor = 6; rem.seed = 5;
  EXPECT(hnsw_add_params(nullptr, rem, 100, 8, 4, q) == 0);                            // the remembered ones
  EXPECT(q.m == 4 && q.m0 == 8 && q.ef_construction == 16 && q.prune_cnt == 3 && q.min_neighbors == 2 && q.scaling_factor == 6 && q.seed == 5);
  p.ef_construction = 40;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == 0 && q.ef_construction == 40 && q.prune_cnt == 3);
  EXPECT(hnsw_add_params(nullptr, none, 100, 8, 0, q) == 0 && q.m0 == 8 && q.m == 50);  // a loaded graph without upper lists
  EXPECT(hnsw_add_params(nullptr, none, 100, 8, 4, q) == 0 && q.m0 == 8 && q.m == 4 && q.prune_cnt == 4 && q.ef_construction == 500);
  p = none; p.m0 = 16;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == ZVEC_HIP_ERR_INVALID_ARGUMENT);     // m0 disagrees with the graph
  EXPECT(hnsw_add_params(&p, rem, 0, 8, 4, q) == 0 && q.m0 == 16);                      // no nodes, no graph to disagree with
  p = none; p.m = 8;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == ZVEC_HIP_ERR_INVALID_ARGUMENT);     // m disagrees with the upper lists
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 0, q) == 0 && q.m == 8);                      // no upper lists yet
  p = none; p.m = 4; p.m0 = 8;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == 0);
  p = none; p.ef_construction = 513;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == ZVEC_HIP_ERR_UNSUPPORTED);
  p = none; p.m0 = 257;
  EXPECT(hnsw_add_params(&p, none, 0, 0, 0, q) == ZVEC_HIP_ERR_UNSUPPORTED);
  p = none; p.m = 129;
  EXPECT(hnsw_add_params(&p, none, 0, 0, 0, q) == ZVEC_HIP_ERR_UNSUPPORTED);
  p = none; p.min_neighbors = 5;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
  p.min_neighbors = 4;
  EXPECT(hnsw_add_params(&p, rem, 100, 8, 4, q) == 0);

  std::vector<uint32_t> lv;
  const uint32_t given[4] = {0, 15, 16, 1};
  EXPECT(hnsw_add_levels(10, 4, given, q, lv) == ZVEC_HIP_ERR_INVALID_ARGUMENT);       // a level of 16 in the middle
  EXPECT(hnsw_add_levels(10, 2, given, q, lv) == 0 && lv.size() == 2 && lv[1] == 15);
  EXPECT(hnsw_add_levels(0xffffffe0ull, 16, given, q, lv) == ZVEC_HIP_ERR_OUT_OF_RANGE && hnsw_add_levels(0xffffffe0ull, 15, nullptr, rem, lv) == 0);
  EXPECT(hnsw_add_levels(~0ull, 2, given, q, lv) == ZVEC_HIP_ERR_OUT_OF_RANGE);
  q.scaling_factor = 4;
  EXPECT(hnsw_add_levels(10, 4, nullptr, q, lv) == ZVEC_HIP_ERR_INVALID_ARGUMENT);     // generated levels want 5 .. 1000
  EXPECT(hnsw_add_levels(1234, 100, nullptr, rem, lv) == 0);
  std::vector<uint32_t> ref(1334);
  EXPECT(hnsw_levels_range(0, 1334, 6, 5, ref.data()) == 0 && std::equal(lv.begin(), lv.end(), ref.begin() + 1234));
}

void capacity_and_stride() {
  EXPECT(hnsw_grow(100, 100, 0) == 100 && hnsw_grow(100, 50, 1000) == 100);            // enough is left alone, a reserve does not move it
  EXPECT(hnsw_grow(100, 101, 0) == 200 && hnsw_grow(100, 500, 0) == 500 && hnsw_grow(0, 1, 0) == 1 && hnsw_grow(0, 7, 600) == 600);
  EXPECT(hnsw_grow(100, 101, 150) == 200);
  uint64_t cap = 0, moves = 0;
  for (uint64_t n = 1; n <= 1000000; ++n) {                                             // one row per call: O(log n) moves
    const uint64_t c2 = hnsw_grow(cap, n, 0);
    EXPECT(c2 >= n && c2 >= cap);
    moves += c2 != cap;
    cap = c2;
  }
  EXPECT(moves <= 21);
  EXPECT(hnsw_reserve_upper(600, 4) == 264 && hnsw_reserve_upper(10, 50) == 10 && hnsw_reserve_upper(1000000, 50) == 1000000 / 49 + 64);
  EXPECT(hnsw_reserve_upper(100, 0) == 100);

  const uint32_t lv[6] = {0, 1, 0, 3, 2, 0};
  uint32_t up[6];
  HnswAddShape sh = hnsw_add_shape(1, 10, lv, 6, up);
  EXPECT(sh.stride == 3 && sh.n_upper == 13 && sh.restride);
  EXPECT(up[0] == 0xffffffffu && up[1] == 10 && up[2] == 0xffffffffu && up[3] == 11 && up[4] == 12 && up[5] == 0xffffffffu);
  sh = hnsw_add_shape(3, 10, lv, 6, nullptr);
  EXPECT(sh.stride == 3 && sh.n_upper == 13 && !sh.restride);
  sh = hnsw_add_shape(0, 0, lv, 1, up);                                                 // level-0 rows on a graph without upper lists
  EXPECT(sh.stride == 0 && sh.n_upper == 0 && !sh.restride);
  sh = hnsw_add_shape(0, 0, lv, 2, up);                                                 // the first upper node makes the table
  EXPECT(sh.stride == 1 && sh.n_upper == 1 && sh.restride && up[1] == 0);
  sh = hnsw_add_shape(2, 5, lv, 0, nullptr);
  EXPECT(sh.stride == 2 && sh.n_upper == 5 && !sh.restride);
}

// a graph grown by random calls: every call's plan equals the restatement from its base; with round_div 0, and with one row per call,
// the rounds of all calls together are the sequential rounds of one build (P1, P2); upper ranks and the stride go on from call to call
void random_sequences() {
  std::mt19937_64 rng(20260321);
  for (int it = 0; it < 3000; ++it) {
    const uint32_t n = 1 + (uint32_t)(rng() % 400);
    const uint32_t div = it % 3 == 0 ? 0 : 1 + (uint32_t)(rng() % 20), mx = 1 + (uint32_t)(rng() % 70);
    const uint32_t m = 1 + (uint32_t)(rng() % 50), m0 = 1 + (uint32_t)(rng() % 100);
    std::vector<uint32_t> lv(n);
    for (uint32_t &v : lv) { const uint64_t r = rng() % 1000; v = r < 700 ? 0 : r < 930 ? 1 : r < 985 ? 2 : (uint32_t)(3 + rng() % 13); }
    const bool single = it % 5 == 1;
    uint32_t base = 0, entry = 0, top = 0, stride = 0, n_upper = 0;
    size_t rounds = 0;
    uint64_t cap = 0;
    std::vector<uint32_t> upper_of(n);
    HnswShape shape;                                                                    // of the graph grown by hnsw_insert_plan
    zvec_hip_hnsw_build_params p{};
    p.m = m; p.m0 = m0; p.ef_construction = 16;
    const uint64_t want_rows = it % 4 == 2 ? n / 2 : 0, want_upper = it % 4 == 2 ? 7 : 0;
    while (base < n) {
      const uint32_t count = single ? 1 : 1 + (uint32_t)(rng() % std::min<uint32_t>(n - base, 150));
      const uint32_t e0 = entry, t0 = top;
      check_call(lv, base, count, div, mx, m0, m, entry, top);
      std::vector<HnswRound> plan;
      std::vector<uint64_t> off;
      uint32_t e1 = e0, t1 = t0;
      hnsw_plan_rounds(base, lv.data() + base, count, div, mx, m0, m, e1, t1, plan, off);
      rounds += plan.size();
      if (div == 0 || single)
        for (const HnswRound &r : plan) EXPECT(r.end == r.first + 1);
      const HnswRoundsNeed need = hnsw_rounds_need(plan, off, base, 4096);
      for (const HnswRound &r : plan) {
        EXPECT(off[r.end - base] - off[r.first - base] <= need.max_slots);
        const uint32_t slice = hnsw_round_slice(r, 4096);
        EXPECT(slice >= 1 && slice <= r.end - r.first && slice * hnsw_round_node_bytes(r.first) <= std::max<uint64_t>(need.max_ws, 1));
        EXPECT(slice == 1 || slice * hnsw_round_node_bytes(r.first) <= 4096);
      }
      const HnswAddShape sh = hnsw_add_shape(stride, n_upper, lv.data() + base, count, upper_of.data() + base);
      uint32_t mxl = stride;
      for (uint32_t i = base; i < base + count; ++i) mxl = std::max(mxl, lv[i]);
      EXPECT(sh.stride == mxl && sh.restride == (mxl > stride));
      stride = sh.stride; n_upper = sh.n_upper;
      EXPECT(top == stride || base + count == 0);                                       // the entry point is on the largest level
      cap = hnsw_grow(cap, (uint64_t)base + count, want_rows);
      EXPECT(cap >= (uint64_t)base + count);
      // the one plan, from the shape the last call left: the same rounds, ranks, stride and capacity as the pieces above
      EXPECT(shape.n == base && shape.entry == e0 && shape.stride == t0);
      HnswInsertPlan pl;
      check_plan(shape, p, want_rows, want_upper, lv.data() + base, count, base ? nullptr : &p, div, mx, 4096, true, pl);
      EXPECT(pl.rounds.size() == plan.size() && pl.after.entry == entry && pl.top == top && pl.after.stride == stride && pl.after.n_upper == n_upper);
      EXPECT(pl.after.cap_rows == cap && pl.after.cap_upper >= n_upper && std::equal(pl.upper_of.begin(), pl.upper_of.end(), upper_of.begin() + base));
      shape = pl.after;
      base += count;
    }
    uint32_t rank = 0;
    for (uint32_t i = 0; i < n; ++i) EXPECT(upper_of[i] == (lv[i] >= 1 ? rank++ : 0xffffffffu));      // the ranks of one build
    EXPECT(rank == n_upper);
    if (div == 0 || single) {                                                           // P1 / P2: the sequential plan
      EXPECT(rounds == n - 1);
      uint32_t e2 = 0, t2 = 0;
      const std::vector<Step> seq = restated(lv, 0, n, 0, mx, e2, t2);
      EXPECT(seq.size() == rounds && e2 == entry && t2 == top);
    }
  }
}

}  // namespace

int main() {
  fixed_cases();
  levels_and_params();
  capacity_and_stride();
  insert_plan_cases();
  random_sequences();
  printf("ok\n");
  return 0;
}
