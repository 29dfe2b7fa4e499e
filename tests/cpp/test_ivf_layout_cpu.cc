// The host's share of an IVF build (zvec_amd/csrc/host/ivf_layout.h: ivf_lpt_owner, IvfLayout::begin / place / finish / store_pos,
// labels_of_offsets, count_sizes) against a model that takes one row at a time: per-list append vectors, and the arithmetic of the
// hand-written build it replaces, restated literally (owner map, layout, cursors, deal order, levels, chunk length).  After every
// call every member of the layout is what the model says; a refused call leaves the layout equal to a copy taken before it, and
// the corrected chunk then goes in.
// Plain host C++, no GPU and no library: g++ -std=c++17 tests/cpp/test_ivf_layout_cpu.cc && ./a.out
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../zvec_amd/csrc/host/ivf_layout.h"

namespace {

int cases = 0;

#define REQUIRE(cond)                                                                       \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      fprintf(stderr, "case %d: %s failed (%s:%d)\n", cases, #cond, __FILE__, __LINE__);    \
      exit(1);                                                                              \
    }                                                                                       \
  } while (0)

constexpr uint32_t TILE_N = 128;

uint64_t rng_state = 1;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

// ---- the model: the fields of the hand-written build and its four functions, a row at a time ----
struct Model {
  uint32_t nlist = 0, shard = 0, nshards = 1;
  std::vector<uint32_t> h_owner, h_size, h_size_global, h_tile0, h_tail, order;
  std::vector<uint64_t> h_cursor, h_dense0, h_row_ids, h_rows_of_largest;
  uint64_t count_local = 0, count_global = 0, local_tiles = 0;
  uint32_t tiles_per_chunk = 8;
  std::vector<std::vector<uint64_t>> lists;      // per list: the global row numbers appended so far, in arrival order
};

void model_lpt_owner(const uint32_t *sizes, uint32_t nlist, uint32_t nshards, uint32_t *owner, uint64_t *rows_out) {
  std::vector<uint64_t> load(nshards, 0), rows(nshards, 0);
  if (nshards <= 1) {
    for (uint32_t l = 0; l < nlist; ++l) { owner[l] = 0; rows[0] += sizes[l]; }
  } else {
    std::vector<uint32_t> order(nlist);
    for (uint32_t l = 0; l < nlist; ++l) order[l] = l;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return sizes[x] > sizes[y]; });
    for (uint32_t i = 0; i < nlist; ++i) {
      const uint32_t l = order[i];
      uint32_t best = 0;
      for (uint32_t g = 1; g < nshards; ++g)
        if (load[g] < load[best]) best = g;
      owner[l] = best;
      load[best] += (sizes[l] + TILE_N - 1) / TILE_N;
      rows[best] += sizes[l];
    }
  }
  if (rows_out) for (uint32_t g = 0; g < nshards; ++g) rows_out[g] = rows[g];
}

int model_begin(Model &h, const uint32_t *sizes_global, uint32_t nlist) {
  h.nlist = nlist;
  h.h_size_global.assign(sizes_global, sizes_global + nlist);
  h.h_owner.assign(nlist, 0);
  model_lpt_owner(sizes_global, nlist, h.nshards, h.h_owner.data(), nullptr);
  h.h_size.assign(nlist, 0);
  uint64_t total = 0;
  for (uint32_t l = 0; l < nlist; ++l) {
    total += sizes_global[l];
    if (h.h_owner[l] == h.shard) h.h_size[l] = sizes_global[l];
  }
  h.h_tile0.assign(nlist, 0);
  h.h_dense0.assign(nlist + 1, 0);
  uint64_t tiles = 0, dense = 0;
  for (uint32_t l = 0; l < nlist; ++l) {
    h.h_tile0[l] = (uint32_t)tiles;
    h.h_dense0[l] = dense;
    tiles += (h.h_size[l] + TILE_N - 1) / TILE_N;
    dense += h.h_size[l];
  }
  h.h_dense0[nlist] = dense;
  h.count_local = dense;
  h.count_global = total;
  h.local_tiles = tiles;
  if (tiles * TILE_N >= 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  h.h_cursor.assign(h.h_dense0.begin(), h.h_dense0.end() - 1);
  h.h_row_ids.assign(dense, 0);
  h.lists.assign(nlist, std::vector<uint64_t>());
  return 0;
}

// (only ever called with a chunk the row-at-a-time lists accept: a refusal half-way is what the layout must not imitate)
void model_add_rows(Model &h, uint64_t n, const uint32_t *labels, const uint64_t *keys, uint64_t first_row, std::vector<uint64_t> &src,
                    std::vector<uint64_t> &dst, std::vector<uint64_t> &kv) {
  src.clear(); dst.clear(); kv.clear();
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t l = labels[i];
    REQUIRE(l < h.nlist);
    if (h.h_owner[l] != h.shard) continue;
    const uint64_t d = h.h_cursor[l];
    REQUIRE(d < h.h_dense0[l + 1]);
    h.h_cursor[l] = d + 1;
    h.h_row_ids[d] = first_row + i;
    src.push_back(i);
    dst.push_back((uint64_t)h.h_tile0[l] * TILE_N + (d - h.h_dense0[l]));
    kv.push_back(keys ? keys[i] : first_row + i);
    // the same row through the per-list append: it lands behind the rows the list holds
    REQUIRE(dst.back() == (uint64_t)h.h_tile0[l] * TILE_N + h.lists[l].size());
    h.lists[l].push_back(first_row + i);
  }
}

// does the per-list append accept the whole chunk?
bool model_accepts(const Model &h, uint64_t n, const uint32_t *labels) {
  std::vector<uint64_t> more(h.nlist, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t l = labels[i];
    if (l >= h.nlist) return false;
    if (h.h_owner[l] != h.shard) continue;
    if (h.lists[l].size() + ++more[l] > h.h_size[l]) return false;
  }
  return true;
}

int model_end(Model &h, uint64_t head_num, uint32_t tpc_knob) {
  const uint32_t nlist = h.nlist;
  for (uint32_t l = 0; l < nlist; ++l)
    if (h.h_cursor[l] != h.h_dense0[l + 1]) return ZVEC_HIP_ERR_NO_READY;
  const uint64_t tiles = h.local_tiles;
  std::vector<uint32_t> order(nlist);
  for (uint32_t l = 0; l < nlist; ++l) order[l] = l;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h.h_size[x] > h.h_size[y]; });
  {
    uint64_t tpc = tiles / (4ull * 256ull * 3ull);
    h.tiles_per_chunk = (uint32_t)std::min<uint64_t>(32, std::max<uint64_t>(4, tpc));
    if (tpc_knob) h.tiles_per_chunk = tpc_knob;
    h.h_tail.assign(nlist, 1);
    uint64_t acc = 0;
    for (uint32_t i = nlist; i-- > 0;) {
      const uint32_t l = order[i];
      if (acc * 4 >= tiles) break;
      h.h_tail[l] = 2;
      acc += (h.h_size[l] + TILE_N - 1) / TILE_N;
    }
    acc = 0;
    for (uint32_t i = 0; i < nlist; ++i) {
      const uint32_t l = order[i];
      if (acc * 100 >= tiles * head_num || h.h_tail[l] == 2) break;
      h.h_tail[l] = 0;
      acc += (h.h_size[l] + TILE_N - 1) / TILE_N;
    }
  }
  h.order = order;
  {
    std::vector<uint32_t> sz(h.h_size);
    std::sort(sz.begin(), sz.end(), std::greater<uint32_t>());
    h.h_rows_of_largest.assign((size_t)nlist + 1, 0);
    for (uint32_t i = 0; i < nlist; ++i) h.h_rows_of_largest[i + 1] = h.h_rows_of_largest[i] + sz[i];
  }
  return 0;
}

// ---- comparisons ----
bool same(const IvfLayout &a, const IvfLayout &b) {
  return a.nlist == b.nlist && a.shard == b.shard && a.nshards == b.nshards && a.owner == b.owner && a.size == b.size &&
         a.size_global == b.size_global && a.tile0 == b.tile0 && a.dense0 == b.dense0 && a.cursor == b.cursor && a.row_ids == b.row_ids &&
         a.order == b.order && a.tail == b.tail && a.rows_of_largest == b.rows_of_largest && a.count_local == b.count_local &&
         a.count_global == b.count_global && a.local_tiles == b.local_tiles && a.tiles_per_chunk == b.tiles_per_chunk;
}

// every member against the model; `finished`: the members finish() makes as well
void check(const IvfLayout &lay, const Model &m, bool finished) {
  REQUIRE(lay.nlist == m.nlist && lay.shard == m.shard && lay.nshards == m.nshards);
  REQUIRE(lay.owner == m.h_owner);
  REQUIRE(lay.size == m.h_size);
  REQUIRE(lay.size_global == m.h_size_global);
  REQUIRE(lay.tile0 == m.h_tile0);
  REQUIRE(lay.dense0 == m.h_dense0);
  REQUIRE(lay.cursor == m.h_cursor);
  REQUIRE(lay.row_ids == m.h_row_ids);
  REQUIRE(lay.count_local == m.count_local && lay.count_global == m.count_global && lay.local_tiles == m.local_tiles);
  for (uint32_t l = 0; l < m.nlist; ++l) {       // the per-list append: list l holds its rows in arrival order
    REQUIRE(lay.cursor[l] - lay.dense0[l] == m.lists[l].size());
    for (size_t j = 0; j < m.lists[l].size(); ++j) REQUIRE(lay.row_ids[lay.dense0[l] + j] == m.lists[l][j]);
  }
  if (finished) {
    REQUIRE(lay.order == m.order);
    REQUIRE(lay.tail == m.h_tail);
    REQUIRE(lay.rows_of_largest == m.h_rows_of_largest);
    REQUIRE(lay.tiles_per_chunk == m.tiles_per_chunk);
  }
}

void check_store_pos(const IvfLayout &lay) {
  uint64_t pos = ~0ull;
  for (uint32_t l = 0; l < lay.nlist; ++l) {
    if (lay.size[l] == 0) continue;
    REQUIRE(lay.store_pos(lay.dense0[l], &pos) && pos == (uint64_t)lay.tile0[l] * TILE_N);
    REQUIRE(lay.store_pos(lay.dense0[l + 1] - 1, &pos) && pos == (uint64_t)lay.tile0[l] * TILE_N + lay.size[l] - 1);
  }
  pos = 12345;
  REQUIRE(!lay.store_pos(lay.count_local, &pos) && pos == 12345);
  REQUIRE(!lay.store_pos(~0ull, &pos) && pos == 12345);
}

// labels of `sizes` rows per list, in an order the seed picks (cyclic over the lists, or shuffled)
std::vector<uint32_t> make_labels(const std::vector<uint32_t> &sizes, bool shuffle) {
  std::vector<uint32_t> left(sizes), labels;
  uint64_t n = 0;
  for (uint32_t s : sizes) n += s;
  labels.reserve(n);
  for (bool any = true; any;) {
    any = false;
    for (uint32_t l = 0; l < left.size(); ++l)
      if (left[l]) { labels.push_back(l); --left[l]; any = true; }
  }
  if (shuffle)
    for (uint64_t i = labels.size(); i > 1; --i) std::swap(labels[i - 1], labels[rnd() % i]);
  return labels;
}

// One whole build of `sizes` as shard `shard` of `nshards`: begin, the rows in chunks of `chunk` (0: one call; a seeded share of the
// chunks is first sent wrong and must be refused), finish.  `with_keys`: keys given, else nullptr.
void build(const std::vector<uint32_t> &sizes, uint32_t shard, uint32_t nshards, uint64_t chunk, bool with_keys, bool shuffle, bool faults,
           uint32_t head_pct, uint32_t tpc_override) {
  ++cases;
  const uint32_t nlist = (uint32_t)sizes.size();
  IvfLayout lay;
  lay.shard = shard; lay.nshards = nshards;
  Model m;
  m.shard = shard; m.nshards = nshards;
  REQUIRE(lay.begin(sizes.data(), nlist) == 0);
  REQUIRE(model_begin(m, sizes.data(), nlist) == 0);
  check(lay, m, false);
  check_store_pos(lay);
  {                                   // the public map is the one begin() used
    std::vector<uint32_t> own(nlist), want(nlist);
    std::vector<uint64_t> rows(nshards), wrows(nshards);
    ivf_lpt_owner(sizes.data(), nlist, nshards, own.data(), rows.data());
    model_lpt_owner(sizes.data(), nlist, nshards, want.data(), wrows.data());
    REQUIRE(own == want && own == lay.owner && rows == wrows && rows[shard] == lay.count_local);
  }
  const std::vector<uint32_t> labels = make_labels(sizes, shuffle);
  const uint64_t n = labels.size();
  std::vector<uint64_t> keys(n);
  for (uint64_t i = 0; i < n; ++i) keys[i] = 1000000007ull * (i + 1) + 5;
  {                                   // count_sizes gives the sizes back and refuses a label that names no list
    std::vector<uint32_t> back;
    REQUIRE(IvfLayout::count_sizes(labels.data(), n, nlist, back) == 0 && back == sizes);
    if (n) {
      std::vector<uint32_t> bad(labels);
      bad[n - 1] = nlist;
      REQUIRE(IvfLayout::count_sizes(bad.data(), n, nlist, back) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
    }
  }
  // one call with every row on a copy: what the chunks together must give
  IvfLayout whole(lay);
  std::vector<uint64_t> wsrc, wdst, wkv;
  REQUIRE(whole.place(labels.data(), n, with_keys ? keys.data() : nullptr, 0, wsrc, wdst, wkv) == 0);

  std::vector<uint64_t> src, dst, kv, msrc, mdst, mkv, csrc, cdst, ckv;
  if (n && lay.count_local != 0) {    // a fill that is short: finish refuses and changes nothing
    const IvfLayout before(lay);
    REQUIRE(lay.finish(head_pct, tpc_override) == ZVEC_HIP_ERR_NO_READY);
    REQUIRE(same(lay, before));
  }
  for (uint64_t o = 0; o < n || o == 0;) {
    uint64_t c = chunk ? std::min<uint64_t>(n - o, 1 + rnd() % chunk) : n - o;
    const uint32_t *lab = labels.data() + o;
    const uint64_t *ks = with_keys ? keys.data() + o : nullptr;
    if (faults && c && rnd() % 3 == 0) {
      std::vector<uint32_t> bad(lab, lab + c);
      const IvfLayout before(lay);
      // (a) the last label names no list
      bad[c - 1] = nlist + rnd() % 3;
      REQUIRE(!model_accepts(m, c, bad.data()));
      REQUIRE(lay.place(bad.data(), c, ks, o, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
      REQUIRE(same(lay, before));
      // (b) an owned list is sent more rows than it was announced with: its free slots plus one, all behind the chunk's own rows
      uint32_t l = rnd() % nlist;
      for (uint32_t t = 0; t < nlist && m.h_owner[l] != shard; ++t) l = (l + 1) % nlist;
      if (m.h_owner[l] == shard) {
        bad.assign(lab, lab + c);
        const uint64_t room = m.h_size[l] - m.lists[l].size();
        uint64_t in_chunk = 0;
        for (uint64_t i = 0; i < c; ++i) in_chunk += lab[i] == l;
        bad.insert(bad.end(), (size_t)(room - in_chunk + 1), l);
        std::vector<uint64_t> bkeys(bad.size(), 7);
        REQUIRE(!model_accepts(m, bad.size(), bad.data()));
        REQUIRE(lay.place(bad.data(), bad.size(), with_keys ? bkeys.data() : nullptr, o, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
        REQUIRE(same(lay, before));
      }
    }
    REQUIRE(model_accepts(m, c, lab));
    REQUIRE(lay.place(lab, c, ks, o, src, dst, kv) == 0);
    model_add_rows(m, c, lab, ks, o, msrc, mdst, mkv);
    REQUIRE(src == msrc && dst == mdst && kv == mkv);
    check(lay, m, false);
    for (uint64_t s : src) csrc.push_back(s + o);
    cdst.insert(cdst.end(), dst.begin(), dst.end());
    ckv.insert(ckv.end(), kv.begin(), kv.end());
    o += c;
    if (c == 0) break;
  }
  REQUIRE(csrc == wsrc && cdst == wdst && ckv == wkv);
  REQUIRE(same(lay, whole));
  if (!with_keys) REQUIRE(ckv == csrc);      // keys == nullptr: the global row number
  for (uint32_t l = 0; l < nlist; ++l)       // a full list takes no further row
    if (m.h_owner[l] == shard) {
      const IvfLayout before(lay);
      REQUIRE(lay.place(&l, 1, nullptr, n, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
      REQUIRE(same(lay, before));
      break;
    }
  REQUIRE(lay.finish(head_pct, tpc_override) == 0);
  REQUIRE(model_end(m, head_pct, tpc_override) == 0);
  check(lay, m, true);
  check_store_pos(lay);
  // the levels: 2 on a suffix of the deal order, 0 on a prefix, the order largest first and stable
  for (uint32_t i = 0; i + 1 < nlist; ++i) {
    const uint32_t a = lay.order[i], b = lay.order[i + 1];
    REQUIRE(lay.size[a] > lay.size[b] || (lay.size[a] == lay.size[b] && a < b));
    REQUIRE(lay.tail[a] <= lay.tail[b]);
  }
  // a new begin() on the finished layout starts over
  REQUIRE(lay.begin(sizes.data(), nlist) == 0);
  REQUIRE(model_begin(m, sizes.data(), nlist) == 0);
  check(lay, m, false);
}

void fixed_cases() {
  const std::vector<std::vector<uint32_t>> shapes = {
      {0, 1, 127, 128, 129, 257},
      {257, 129, 128, 127, 1, 0},
      {128, 128, 128, 128, 128, 128, 128, 128, 128},      // owner ties
      {5, 5, 5, 5},
      {0, 0, 0},                                             // an all-empty index
      {130, 0, 5},
      {1},
      {0},
      {300, 2, 300, 2, 300, 2, 300, 2, 300, 2, 300, 2, 17},
  };
  const uint32_t shards[] = {1, 2, 3, 8}, heads[] = {0, 50, 75}, tpcs[] = {0, 7};
  for (const auto &sizes : shapes)
    for (uint32_t nshards : shards)
      for (uint32_t shard = 0; shard < nshards; ++shard)
        for (uint32_t head : heads)
          for (uint32_t tpc : tpcs) {
            build(sizes, shard, nshards, 0, true, false, false, head, tpc);
            build(sizes, shard, nshards, 37, false, true, true, head, tpc);
          }
  // enough tiles for the adaptive chunk length to leave its floor: 64 lists of ~40 000 rows, 20 000 tiles
  {
    std::vector<uint32_t> sizes(64);
    for (uint32_t l = 0; l < 64; ++l) sizes[l] = 40000 + 13 * l;
    build(sizes, 0, 1, 100000, false, false, false, 50, 0);
  }
}

// Positions are 32-bit: a shard of 0xffffffff padded rows or more is refused, and nothing is allocated per row for it
void range_cases() {
  ++cases;
  IvfLayout lay;
  const std::vector<uint32_t> small = {3, 4};
  REQUIRE(lay.begin(small.data(), 2) == 0);
  const IvfLayout before(lay);
  const uint32_t huge = 0xffffffffu;
  REQUIRE(lay.begin(&huge, 1) == ZVEC_HIP_ERR_OUT_OF_RANGE);
  REQUIRE(same(lay, before));
  const std::vector<uint32_t> three = {0x60000000u, 0x60000000u, 0x60000000u};
  REQUIRE(lay.begin(three.data(), 3) == ZVEC_HIP_ERR_OUT_OF_RANGE);
  REQUIRE(same(lay, before));
  const uint32_t edge = 0xffffffffu - 128;        // 0x1ffffff tiles: 0xffffff80 padded rows, the last size that fits
  REQUIRE(ivf_tiles(edge) * 128 == 0xffffff80ull);
  // the shard that does not own the huge list holds nothing and is laid out
  IvfLayout other;
  other.shard = 1; other.nshards = 2;
  REQUIRE(other.begin(&huge, 1) == 0);
  REQUIRE(other.count_local == 0 && other.count_global == huge && other.local_tiles == 0 && other.row_ids.empty() && other.owner[0] == 0);
  REQUIRE(other.finish(50, 0) == 0);
  REQUIRE(ivf_tiles(0) == 0 && ivf_tiles(1) == 1 && ivf_tiles(128) == 1 && ivf_tiles(129) == 2 && ivf_tiles(huge) == 0x2000000ull);
}

// The two refusals by hand: sizes {130, 0, 5}, list 0 crossing a tile
void refusal_cases() {
  ++cases;
  const std::vector<uint32_t> sizes = {130, 0, 5};
  IvfLayout lay;
  REQUIRE(lay.begin(sizes.data(), 3) == 0);
  REQUIRE(lay.local_tiles == 3 && lay.tile0 == (std::vector<uint32_t>{0, 2, 2}) && lay.dense0 == (std::vector<uint64_t>{0, 130, 130, 135}));
  std::vector<uint64_t> src, dst, kv;
  std::vector<uint32_t> lab = {0, 2, 0, 7};                  // no list 7, as the LAST row: the three rows in front are not stored
  IvfLayout before(lay);
  REQUIRE(lay.place(lab.data(), 4, nullptr, 0, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT && same(lay, before));
  lab = {2, 2, 2, 2, 0, 2, 2};                               // six rows for the five of list 2: the call's own rows overflow it
  REQUIRE(lay.place(lab.data(), 7, nullptr, 0, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT && same(lay, before));
  lab = {1};                                                 // a list announced empty takes no row
  REQUIRE(lay.place(lab.data(), 1, nullptr, 0, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT && same(lay, before));
  lab = {2, 2, 2, 2, 0, 2};                                  // corrected
  REQUIRE(lay.place(lab.data(), 6, nullptr, 10, src, dst, kv) == 0);
  REQUIRE(src == (std::vector<uint64_t>{0, 1, 2, 3, 4, 5}) && dst == (std::vector<uint64_t>{256, 257, 258, 259, 0, 260}) &&
          kv == (std::vector<uint64_t>{10, 11, 12, 13, 14, 15}));
  before = lay;
  lab = {0, 2};                                              // list 2 is full now: one row overflows it, list 0's row in front stays out
  REQUIRE(lay.place(lab.data(), 2, nullptr, 16, src, dst, kv) == ZVEC_HIP_ERR_INVALID_ARGUMENT && same(lay, before));
  lab.assign(129, 0);
  REQUIRE(lay.place(lab.data(), 129, nullptr, 16, src, dst, kv) == 0 && dst.front() == 1 && dst.back() == 129);
  REQUIRE(lay.finish(50, 0) == 0);
  REQUIRE(lay.row_ids[0] == 14 && lay.row_ids[1] == 16 && lay.row_ids[129] == 144 && lay.row_ids[130] == 10 && lay.row_ids[134] == 15);
}

void offsets_cases() {
  ++cases;
  std::vector<uint32_t> labels = {9, 9};
  const std::vector<uint64_t> offs = {0, 2, 2, 5, 6};
  REQUIRE(IvfLayout::labels_of_offsets(offs.data(), 4, labels) == 0);
  REQUIRE((labels == std::vector<uint32_t>{0, 0, 2, 2, 2, 3}));
  const std::vector<uint64_t> down = {0, 4, 2, 3};         // descends: refused before a label is written (3 rows, offset 4)
  labels = {9, 9};
  REQUIRE(IvfLayout::labels_of_offsets(down.data(), 3, labels) == ZVEC_HIP_ERR_INVALID_ARGUMENT);
  REQUIRE((labels == std::vector<uint32_t>{9, 9}));
  const std::vector<uint64_t> none = {0, 0};
  REQUIRE(IvfLayout::labels_of_offsets(none.data(), 1, labels) == 0 && labels.empty());
}

void random_cases(int count) {
  const uint32_t pick[] = {0, 1, 127, 128, 129, 257};
  for (int c = 0; c < count; ++c) {
    rng_state = 0x9e3779b97f4a7c15ull * (uint64_t)(c + 1);
    const uint32_t nlist = 1 + rnd() % 24;
    std::vector<uint32_t> sizes(nlist);
    const uint32_t mode = rnd() % 4;
    for (uint32_t l = 0; l < nlist; ++l)
      sizes[l] = mode == 0 ? pick[rnd() % 6] : mode == 1 ? rnd() % 300 : mode == 2 ? 64 * (rnd() % 3) : (rnd() % 5 == 0 ? 0 : 1 + rnd() % 140);
    const uint32_t nshards = 1 + rnd() % 8, shard = rnd() % nshards;
    const uint32_t heads[] = {0, 25, 50, 75};
    build(sizes, shard, nshards, rnd() % 2 ? 1 + rnd() % 200 : 0, rnd() % 2, rnd() % 4 != 0, rnd() % 2, heads[rnd() % 4], rnd() % 3 == 0 ? 1 + rnd() % 9 : 0);
  }
}

}  // namespace

int main() {
  fixed_cases();
  range_cases();
  refusal_cases();
  offsets_cases();
  random_cases(3000);
  printf("%d cases\nok\n", cases);
  return 0;
}
