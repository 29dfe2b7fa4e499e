// hnsw_add_plan.h — the host's share of inserting nodes into an HNSW graph, for the build (zvec_hip_hnsw_build, base 0) and the append
// (zvec_hip_hnsw_add, base = the nodes already there): the levels of a range of positions, the parameters a call runs with, the rounds
// from a base with the request offsets of the new nodes only, the capacity steps and the stride of the upper table; and all of them
// in the order both entries run them, as one plan (hnsw_insert_plan).  DESIGN §3c "Building" and "Appending".  Nothing of HIP:
// tests/cpp/test_hnsw_add_plan_cpu.cc.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../../include/zvec_hip.h"      // (the error codes, zvec_hip_hnsw_build_params)

constexpr uint32_t HNSW_PLAN_MAX_LEVEL = ZVEC_HIP_HNSW_BUILD_MAX_LEVEL;
constexpr uint32_t HNSW_PLAN_MAX_EF = 512, HNSW_PLAN_MAX_M0 = 256, HNSW_PLAN_MAX_M = 128;      // (the kernels' limits, zvk_hnsw*.hip.h)
constexpr uint64_t HNSW_PLAN_MAX_NODES = 0xfffffff0ull;                                        // node ids are 32-bit, IDX_NONE reserved

// HnswAlgorithm::get_random_level (hnsw_algorithm.h) in integer arithmetic for the positions first .. first + count - 1: the level of a
// position does not depend on which call asks for it
inline int hnsw_levels_range(uint64_t first, uint64_t count, uint32_t scaling_factor, uint64_t seed, uint32_t *out) {
  if (count && !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (scaling_factor < 5 || scaling_factor > 1000) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  // thr[k - 1] = ceil(2^53 / sf^k): r * sf^k < 2^53 <=> r < thr[k - 1]; once sf^k >= 2^53 only r == 0 passes
  uint64_t thr[HNSW_PLAN_MAX_LEVEL];
  uint64_t pw = 1;
  for (uint32_t k = 0; k < HNSW_PLAN_MAX_LEVEL; ++k) {
    if (pw < (1ull << 53)) pw *= scaling_factor;
    thr[k] = ((1ull << 53) + pw - 1) / pw;
  }
  for (uint64_t j = 0; j < count; ++j) {
    const uint64_t i = first + j;
    uint64_t z = seed + i * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    const uint64_t r = (z ^ (z >> 31)) >> 11;
    uint32_t level = 0;
    while (level < HNSW_PLAN_MAX_LEVEL && r < thr[level]) ++level;
    out[j] = level;
  }
  return 0;
}

// What an insertion runs with.  p: the caller's (nullable); rem: what the handle remembers of its last build, all zero on a handle that
// a load filled.  A field left 0 takes the remembered value, and the reference's default where nothing is remembered (m 50, m0 2m,
// ef_construction 500, prune_cnt m, scaling_factor m).  A graph with n nodes fixes m0; one with upper lists (g_m != 0) fixes m.
inline int hnsw_add_params(const zvec_hip_hnsw_build_params *p, const zvec_hip_hnsw_build_params &rem, uint64_t n, uint32_t g_m0,
                           uint32_t g_m, zvec_hip_hnsw_build_params &q) {
  q = zvec_hip_hnsw_build_params();
  if (p) q = *p;
  if (n && q.m0 && q.m0 != g_m0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n && g_m && q.m && q.m != g_m) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (q.m == 0) q.m = n && g_m ? g_m : rem.m ? rem.m : 50;
  if (q.m0 == 0) q.m0 = n ? g_m0 : rem.m0 ? rem.m0 : 2 * q.m;
  if (q.ef_construction == 0) q.ef_construction = rem.ef_construction ? rem.ef_construction : 500;
  if (q.prune_cnt == 0) q.prune_cnt = rem.prune_cnt ? rem.prune_cnt : q.m;
  if (q.min_neighbors == 0) q.min_neighbors = rem.min_neighbors;
  if (q.scaling_factor == 0) q.scaling_factor = rem.scaling_factor ? rem.scaling_factor : q.m;
  if (q.seed == 0) q.seed = rem.seed;
  if (q.ef_construction > HNSW_PLAN_MAX_EF || q.m0 > HNSW_PLAN_MAX_M0 || q.m > HNSW_PLAN_MAX_M) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (q.min_neighbors > std::min(q.m, q.m0)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return 0;
}

// The levels of the count new nodes behind n: the caller's (each at most 15), or generated for their global positions.
inline int hnsw_add_levels(uint64_t n, uint64_t count, const uint32_t *levels, const zvec_hip_hnsw_build_params &q, std::vector<uint32_t> &lv) {
  if (n + count >= HNSW_PLAN_MAX_NODES || n + count < n) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  lv.resize((size_t)count);
  if (!levels) return hnsw_levels_range(n, count, q.scaling_factor, q.seed, lv.data());
  for (uint64_t i = 0; i < count; ++i) {
    if (levels[i] > HNSW_PLAN_MAX_LEVEL) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    lv[(size_t)i] = levels[i];
  }
  return 0;
}

struct HnswRound { uint32_t first, end, entry, top; };

// The rounds that insert the nodes base .. base + count - 1 (lv: their levels) into a graph of base nodes whose entry point and top
// level are entry / top; both leave as they are after the last round.  With s nodes in the graph a round takes [s, e), e - s =
// clamp(s / round_div, 1, round_max), cut at base + count; a node above top is a round of its own and becomes the entry point after it
// (add_node:73-78).  On an empty graph (base == 0) node 0 is the seed and has no round.  req_off[count + 1]: the first request slot of
// every new node, counted from node `base`: m0 slots for level 0 and m for every level the node is searched on above it.
inline void hnsw_plan_rounds(uint32_t base, const uint32_t *lv, uint32_t count, uint32_t round_div, uint32_t round_max, uint32_t m0,
                             uint32_t m, uint32_t &entry, uint32_t &top, std::vector<HnswRound> &plan, std::vector<uint64_t> &req_off) {
  const uint64_t n = (uint64_t)base + count;
  plan.clear();
  req_off.assign((size_t)count + 1, 0);
  uint32_t s = base;
  if (base == 0) {
    entry = 0;
    top = count ? lv[0] : 0;
    s = 1;
  }
  while (s < n) {
    uint32_t e;
    const bool own = lv[s - base] > top;
    if (own) {
      e = s + 1;
    } else {
      const uint32_t size = round_div == 0 ? 1u : std::min(std::max(s / round_div, 1u), round_max);
      e = (uint32_t)std::min<uint64_t>((uint64_t)s + size, n);
      for (uint32_t j = s + 1; j < e; ++j)
        if (lv[j - base] > top) { e = j; break; }
    }
    plan.push_back({s, e, entry, top});
    for (uint32_t i = s; i < e; ++i)
      req_off[(size_t)(i - base) + 1] = req_off[i - base] + m0 + (uint64_t)std::min(lv[i - base], top) * m;
    if (own) { entry = s; top = lv[s - base]; }
    s = e;
  }
}

// The insert phase of a round goes in slices of nodes whose workspace stays within `budget` bytes ("hnsw_ws_bytes"): a node's share is
// ceil(s / 32) words of visited bits, and 8 * s bytes of candidate region once s > 1024 nodes are in the graph (HNSW_C_LDS).
constexpr uint32_t HNSW_PLAN_C_LDS = 1024;
inline uint64_t hnsw_round_node_bytes(uint32_t s) { return (uint64_t)((s + 31) / 32) * 4 + (s > HNSW_PLAN_C_LDS ? (uint64_t)s * 8 : 0); }
inline uint32_t hnsw_round_slice(const HnswRound &r, uint64_t budget) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(r.end - r.first, budget / hnsw_round_node_bytes(r.first)));
}

// What the rounds of a plan need at most: request slots of one round, workspace of one slice; and how many rounds hold more than one
// node (they sort and group their requests; a round of one node does not)
struct HnswRoundsNeed { uint64_t max_slots = 0, max_ws = 0; uint32_t multi = 0; };
inline HnswRoundsNeed hnsw_rounds_need(const std::vector<HnswRound> &plan, const std::vector<uint64_t> &req_off, uint32_t base, uint64_t budget) {
  HnswRoundsNeed need;
  for (const HnswRound &r : plan) {
    need.max_slots = std::max(need.max_slots, req_off[r.end - base] - req_off[r.first - base]);
    need.max_ws = std::max(need.max_ws, hnsw_round_slice(r, budget) * hnsw_round_node_bytes(r.first));
    if (r.end - r.first > 1) ++need.multi;
  }
  return need;
}

// Capacity steps: never below the need, never shrinking, at least what a reserve asked for, and doubling when the arrays must move.
inline uint64_t hnsw_grow(uint64_t cap, uint64_t need, uint64_t reserved) {
  if (need <= cap) return cap;
  return std::max(std::max(need, reserved), 2 * cap);
}

// the upper nodes zvec_hip_hnsw_reserve sets aside for `rows` rows when it is told none: P(level >= 1) = 1 / scaling_factor, so
// rows / (scaling_factor - 1) is above the expectation by the factor sf / (sf - 1); plus 64, at most rows
inline uint64_t hnsw_reserve_upper(uint64_t rows, uint32_t scaling_factor) {
  const uint64_t sf = std::max<uint32_t>(scaling_factor, 2);
  return std::min(rows, rows / (sf - 1) + 64);
}

// What a call does to the upper table: upper_of[i] is the rank of i among the nodes of level >= 1, so the new nodes take the ranks
// behind n_upper; the stride is the largest level, so the table is re-strided (or made) once, before the call's first round, when the
// call holds a node above the stride it finds.
struct HnswAddShape {
  uint32_t stride = 0;          // after the call
  uint32_t n_upper = 0;         // after the call
  bool restride = false;        // stride > the one found (a graph without upper lists has stride 0)
};
inline HnswAddShape hnsw_add_shape(uint32_t old_stride, uint32_t old_n_upper, const uint32_t *lv, uint64_t count, uint32_t *upper_of) {
  HnswAddShape sh;
  sh.stride = old_stride;
  sh.n_upper = old_n_upper;
  for (uint64_t i = 0; i < count; ++i) {
    sh.stride = std::max(sh.stride, lv[i]);
    const uint32_t rank = lv[i] >= 1 ? sh.n_upper++ : 0xffffffffu;
    if (upper_of) upper_of[i] = rank;
  }
  sh.restride = sh.stride > old_stride;
  return sh;
}

// The plain numbers of a graph: what the arrays hold and what they have room for.  stride: of the upper table, the largest level
// (zvec_hip_hnsw_info's max_level), 0 without upper lists; cap_rows / cap_upper: rows / nodes of level >= 1 the arrays take before
// they must move.  All zero: no graph.
struct HnswShape {
  uint64_t n = 0, cap_rows = 0, cap_upper = 0;
  uint32_t m0 = 0, m = 0, stride = 0, n_upper = 0, entry = 0;
};

// A shape as a handle keeps it: without rows no entry point and no upper lists; without upper lists no m, no stride, no upper nodes
// and no room for any.
inline HnswShape hnsw_shape_kept(HnswShape s) {
  if (s.n == 0) s.entry = s.stride = 0;
  if (s.stride == 0) { s.m = s.n_upper = 0; s.cap_upper = 0; }
  return s;
}

// Everything the host decides about one insertion of `count` nodes behind the `base` a graph holds, before the device is touched.
struct HnswInsertPlan {
  zvec_hip_hnsw_build_params q{};       // what the call runs with
  uint32_t base = 0, count = 0;
  std::vector<uint32_t> lv, upper_of;   // [count] levels and ranks in the upper table of the new nodes
  std::vector<HnswRound> rounds;
  std::vector<uint64_t> req_off;        // [count + 1]
  HnswRoundsNeed need;
  uint64_t budget = 0;                  // the workspace the slices of a round stay within
  HnswShape after;                      // the graph after the call; cap_*: what the arrays grow to (hnsw_grow)
  uint32_t top = 0;                     // the entry point's level after the call
  bool restride = false;                // the upper table is made, or re-strided, before the first round
};

// The prelude of zvec_hip_hnsw_build (found: all zero, rem: all zero, want_*: 0, append: false) and of zvec_hip_hnsw_add (found: the
// graph, or all zero on a handle without nodes; rem: the handle's remembered parameters; want_*: what a reserve asked for; append:
// true).  The two entries order their refusals differently where two faults coincide, and each keeps its order: a build tests the
// node range before the rows and plans an empty call like any other (so it still refuses a scaling_factor no level can be generated
// with); an add tests the rows first, the range with the levels, and answers count == 0 with an empty plan once the parameters stand.
// A refused call leaves `out` as it was.
inline int hnsw_insert_plan(const HnswShape &found, const zvec_hip_hnsw_build_params &rem, uint64_t want_rows, uint64_t want_upper,
                            uint64_t count, bool have_rows, const zvec_hip_hnsw_build_params *p, const uint32_t *levels, uint32_t round_div,
                            uint32_t round_max, uint64_t budget, bool append, HnswInsertPlan &out) {
  HnswInsertPlan pl;
  int rc = hnsw_add_params(p, rem, found.n, found.m0, found.m, pl.q);
  if (rc) return rc;
  if (pl.q.m0 == 0) return ZVEC_HIP_ERR_UNSUPPORTED;       // (a loaded graph without level-0 lists takes no node)
  if (!append && count >= HNSW_PLAN_MAX_NODES) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  if (count && !have_rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  pl.after = found;
  pl.top = found.stride;                // (the entry point of a graph is on its largest level)
  pl.budget = budget;
  if (append && count == 0) { out = std::move(pl); return 0; }
  rc = hnsw_add_levels(found.n, count, levels, pl.q, pl.lv);
  if (rc) return rc;
  pl.base = (uint32_t)found.n;
  pl.count = (uint32_t)count;
  uint32_t entry = found.entry;
  hnsw_plan_rounds(pl.base, pl.lv.data(), pl.count, round_div, round_max, pl.q.m0, pl.q.m, entry, pl.top, pl.rounds, pl.req_off);
  pl.upper_of.resize(pl.count);
  const HnswAddShape sh = hnsw_add_shape(found.stride, found.n_upper, pl.lv.data(), pl.count, pl.upper_of.data());
  pl.need = hnsw_rounds_need(pl.rounds, pl.req_off, pl.base, budget);
  if (pl.need.max_slots >= (1ull << 31)) return ZVEC_HIP_ERR_UNSUPPORTED;       // (group starts are 32-bit, the sort counts in int)
  pl.restride = sh.restride;
  pl.after.n = found.n + count;
  pl.after.m0 = pl.q.m0;
  pl.after.m = sh.stride ? pl.q.m : 0;
  pl.after.stride = sh.stride;
  pl.after.n_upper = sh.n_upper;
  pl.after.entry = entry;
  pl.after.cap_rows = hnsw_grow(found.cap_rows, pl.after.n, want_rows);
  pl.after.cap_upper = sh.stride ? hnsw_grow(found.cap_upper, sh.n_upper, want_upper) : 0;
  out = std::move(pl);
  return 0;
}
