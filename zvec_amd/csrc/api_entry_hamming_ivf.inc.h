// api_entry_hamming_ivf.inc.h — C ABI entry points: binary rows under the Hamming metric through inverted lists (zvec_hip_bivf_*;
// inside extern "C").  Device code: zvk_hamming_ivf.hip.h.  A handle family of its own beside zvec_hip_ivf_s, which keeps refusing
// binary rows.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

struct zvec_hip_bivf_s {
  int device = 0;
  int dtype = 0;
  bool loaded = false;
  uint32_t nlist = 0;
  uint64_t count = 0;
  uint32_t max_tiles = 1;              // the most tiles any list touches (bounds the tile runs a list is cut into)
  Store cent;                          // centroids as a flat binary store
  Store lists;                         // the rows in list order, no padding between lists: position == list-order position
  Scoped<uint32_t> d_off;              // [nlist + 1] list offsets
  std::vector<uint64_t> h_off;         // ... on the host (export)
  std::vector<uint64_t> h_row_ids;     // original row of every position (build); empty: the identity (load)
  std::vector<uint32_t> h_cent;        // [nlist][words]
  Scoped<float> frows;                 // optional: the documents' fp32 rows [count][fdim] in list order (zvec_hip_bivf_build_fp32 / _attach_rows)
  uint32_t fdim = 0;                   // ... their dimension (0: no rows) and the metric of the re-score (L2 or IP)
  int fmetric = 0;
  zvec_hip_ctx_s *defctx = nullptr;
  std::mutex mu;                       // serialises the calls that change the index or use defctx's workspace
  FairSharedMutex rw;                  // searches hold it shared, load and build exclusive (as zvec_hip_flat_s); a context's mutex is taken first
  ~zvec_hip_bivf_s() { delete defctx; }
};

int zvec_hip_bivf_create(uint32_t dim_bits, int dtype, int device, zvec_hip_bivf_t *out) {
  if (!out || dim_bits == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype < ZVEC_HIP_DT_FP32 || dtype > ZVEC_HIP_DT_BINARY64) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (!dtype_is_binary(dtype)) return ZVEC_HIP_ERR_MISMATCH;          // (the metric is Hamming: zvec_hip_flat_create's pairing rule)
  if (dim_bits % (dtype == ZVEC_HIP_DT_BINARY64 ? 64u : 32u) != 0 || dim_bits > (1u << 20)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = nullptr;
  ZRET(ctx_new(device, &c));
  zvec_hip_bivf_s *h = new (std::nothrow) zvec_hip_bivf_s();
  if (!h) { ctx_free(c); return ZVEC_HIP_ERR_NO_MEMORY; }
  h->device = device; h->dtype = dtype; h->defctx = c;
  h->cent.configure(dim_bits, ZVEC_HIP_METRIC_HAMMING, dtype);
  h->lists.configure(dim_bits, ZVEC_HIP_METRIC_HAMMING, dtype);
  *out = h;
  return 0;
}

int zvec_hip_bivf_destroy(zvec_hip_bivf_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
  return 0;
}

// the exact distances of the prepared queries [0, m) of `c` to every centroid: [m][stride] in c->coarse_scores
static int bivf_centroid_scores(zvec_hip_bivf_s *h, zvec_hip_ctx_s *c, uint32_t m, hipStream_t s, const float **dump, uint32_t *stride) {
  const uint32_t ctiles = (h->nlist + TILE_N - 1) / TILE_N;
  ZRET(c->coarse_scores.ensure((size_t)m * ctiles * TILE_N * sizeof(float)));
  HamScanArgs d{};
  d.base = reinterpret_cast<const uint32_t *>(h->cent.base); d.queries = c->qpad.as<uint32_t>(); d.cpr = h->cent.bin_chunks();
  d.k = 1; d.threshold = FLT_MAX; d.nq = m; d.n = h->nlist; d.ntiles = ctiles; d.tiles_per_chunk = 1; d.nchunks = ctiles;
  d.nqblocks = (m + HAM_QB - 1) / HAM_QB; d.gtau = c->gtau.as<uint32_t>();
  d.dump = c->coarse_scores.as<float>(); d.dump_stride = ctiles * TILE_N;
  ZRET(launch_hamming_scan<true>(d, d.nchunks * d.nqblocks, s));
  *dump = d.dump;
  *stride = d.dump_stride;
  return 0;
}

// d_labels[i] = the centroid nearest to plain row i by (distance, index): the coarse path with nprobe = 1.  The caller holds c->mu.
static int bivf_label(zvec_hip_bivf_s *h, zvec_hip_ctx_s *c, const void *d_rows, uint64_t n, uint32_t *d_labels, hipStream_t s) {
  const StoreView &st = h->cent;
  const uint32_t ctiles = (h->nlist + TILE_N - 1) / TILE_N;
  const uint32_t sub = std::min<uint32_t>(dense_sub_batch(n, (uint64_t)ctiles * TILE_N), 1u << 20);
  for (uint64_t r0 = 0; r0 < n; r0 += sub) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(sub, n - r0);
    ZRET(prep_queries(c, st, static_cast<const char *>(d_rows) + (size_t)r0 * st.row_bytes(), m, FLT_MAX, s));
    BivfSelectArgs a{};
    ZRET(bivf_centroid_scores(h, c, m, s, &a.dump, &a.dump_stride));
    a.nq = m; a.nlist = h->nlist; a.np = 1; a.probe_idx = d_labels + r0;
    hipLaunchKernelGGL(bivf_probe_select_kernel, dim3((m + 3) / 4), dim3(256), 0, s, a);
    ZCHK(hipGetLastError());
  }
  return 0;
}

// Everything a load or a build replaces, under the three locks (h->mu, the built-in context's, h->rw exclusively): the index is
// unloaded while it lives and loaded again by done(0).
struct BivfWrite {
  zvec_hip_bivf_s *const h;
  explicit BivfWrite(zvec_hip_bivf_s *h_) : h(h_), g(h_->mu), gc(h_->defctx->mu), w(h_->rw) { h->loaded = false; }
  // `nlist` centroids (plain device words) become the centroid store
  int set_centroids(const uint32_t *d_cent, uint32_t nlist, hipStream_t s) {
    h->cent.release();
    h->cent.n = 0;
    h->nlist = nlist;
    return store_append_dev(h->cent, d_cent, nlist, nullptr, s);
  }
  // the list offsets and what follows from them
  int set_offsets(const std::vector<uint64_t> &off, hipStream_t s) {
    h->h_off = off;
    h->count = off.back();
    std::vector<uint32_t> o32(off.begin(), off.end());
    h->max_tiles = 1;
    for (size_t l = 0; l + 1 < o32.size(); ++l)
      if (o32[l + 1] > o32[l]) h->max_tiles = std::max(h->max_tiles, bivf_list_cut(o32[l], o32[l + 1], 1).nt);
    ZRET(h->d_off.alloc(o32.size()));
    ZCHK(hipMemcpyAsync(h->d_off, o32.data(), o32.size() * 4, hipMemcpyHostToDevice, s));
    ZCHK(hipStreamSynchronize(s));       // (o32 is a local)
    return 0;
  }
  void clear_rows() {
    h->lists.release();
    h->lists.n = 0;
    h->frows.release();                  // (the fp32 rows belong to the rows that go)
    h->fdim = 0;
  }
  int done(int rc, hipStream_t s) {
    const hipError_t he = hipStreamSynchronize(s);
    if (rc == 0 && he != hipSuccess) rc = ZVEC_HIP_ERR_RUNTIME;
    h->loaded = rc == 0;
    h->defctx->bivf_count = 0;
    h->defctx->bivf_cand_count = 0;
    return rc;
  }

 private:
  std::lock_guard<std::mutex> g, gc;
  std::unique_lock<FairSharedMutex> w;
};

int zvec_hip_bivf_load(zvec_hip_bivf_t h, const void *centroids, uint32_t nlist, const uint64_t *list_offsets, const void *rows,
                       const uint64_t *keys) {
  if (!h || !centroids || nlist == 0 || !list_offsets) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (list_offsets[0] != 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  for (uint32_t l = 0; l < nlist; ++l)
    if (list_offsets[l + 1] < list_offsets[l]) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const uint64_t n = list_offsets[nlist];
  if (n && !rows) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n >= 0xfffffff0ull) return ZVEC_HIP_ERR_OUT_OF_RANGE;       // positions are 32-bit (IDX_NONE reserved)
  ZCHK(hipSetDevice(h->device));
  BivfWrite w(h);
  hipStream_t s = h->defctx->own;
  const size_t rb = h->lists.row_bytes(), words = h->lists.bin_words();
  auto body = [&]() -> int {
    Scoped<uint32_t> d_cent;
    ZRET(d_cent.alloc((size_t)nlist * words));
    ZCHK(hipMemcpyAsync(d_cent, centroids, (size_t)nlist * rb, hipMemcpyHostToDevice, s));
    ZRET(w.set_centroids(d_cent, nlist, s));
    ZRET(w.set_offsets(std::vector<uint64_t>(list_offsets, list_offsets + nlist + 1), s));     // (synchronises: d_cent may go)
    h->h_cent.assign(static_cast<const uint32_t *>(centroids), static_cast<const uint32_t *>(centroids) + (size_t)nlist * words);
    h->h_row_ids.clear();
    w.clear_rows();
    // the rows through the device in slices of <= 1 GiB, as zvec_hip_flat_append stages them
    const uint64_t rows_per = std::max<uint64_t>(1, ((uint64_t)1 << 30) / (uint64_t)rb);
    DevBuf tmp, tk;
    for (uint64_t o = 0; o < n; o += rows_per) {
      const uint64_t m = std::min(rows_per, n - o);
      ZRET(tmp.ensure((size_t)m * rb));
      if (keys) ZRET(tk.ensure((size_t)m * 8));
      ZCHK(hipMemcpyAsync(tmp.p, static_cast<const char *>(rows) + (size_t)o * rb, (size_t)m * rb, hipMemcpyHostToDevice, s));
      if (keys) ZCHK(hipMemcpyAsync(tk.p, keys + o, (size_t)m * 8, hipMemcpyHostToDevice, s));
      ZRET(store_append_dev(h->lists, tmp.p, m, keys ? tk.as<uint64_t>() : nullptr, s));
      ZCHK(hipStreamSynchronize(s));
    }
    return 0;
  };
  return w.done(body(), s);
}

// nlist distinct row numbers out of n: a partial Fisher-Yates shuffle (pick i swaps places with one of i .. n - 1) driven by
// splitmix64 seeded with `seed`, the draw reduced by `% (n - i)`.  Portable: the same arguments give the same rows everywhere.
static std::vector<uint64_t> bivf_initial_rows(uint64_t n, uint32_t nlist, uint64_t seed) {
  uint64_t state = seed;
  auto next = [&]() {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  std::vector<std::pair<uint64_t, uint64_t>> moved;       // (place, the row number now at it): at most nlist entries
  auto at = [&](uint64_t p) {
    for (const auto &e : moved)
      if (e.first == p) return e.second;
    return p;
  };
  auto put = [&](uint64_t p, uint64_t v) {
    for (auto &e : moved)
      if (e.first == p) { e.second = v; return; }
    moved.emplace_back(p, v);
  };
  std::vector<uint64_t> out(nlist);
  for (uint32_t i = 0; i < nlist; ++i) {
    const uint64_t j = i + next() % (n - i);
    const uint64_t vi = at(i), vj = at(j);
    out[i] = vj;
    put(j, vi);
  }
  return out;
}

// the build proper: plain DEVICE rows -> centroids, labels, packed lists.  The caller holds the write scope.
// perm_out: receives the packing permutation on the device (list-order position -> original row)
static int bivf_build_locked(BivfWrite &w, const void *d_rows, uint64_t n, const uint64_t *keys, uint32_t nlist, uint32_t iters,
                             uint64_t seed, hipStream_t s, Scoped<uint64_t> *perm_out = nullptr) {
  zvec_hip_bivf_s *h = w.h;
  zvec_hip_ctx_s *c = h->defctx;
  const uint32_t words = h->lists.bin_words(), dim = words * 32;
  const uint32_t *rows = static_cast<const uint32_t *>(d_rows);
  // 1. initial centroids: nlist distinct rows
  const std::vector<uint64_t> init = bivf_initial_rows(n, nlist, seed);
  Scoped<uint64_t> d_init;
  Scoped<uint32_t> d_cent, d_labels, d_ones, d_members;
  ZRET(d_init.alloc(nlist));
  ZRET(d_cent.alloc((size_t)nlist * words));
  ZRET(d_labels.alloc(n));
  ZRET(d_ones.alloc((size_t)nlist * dim));
  ZRET(d_members.alloc(nlist));
  ZCHK(hipMemcpyAsync(d_init, init.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, s));
  const uint64_t cwords = (uint64_t)nlist * words;
  hipLaunchKernelGGL(bivf_gather_rows_kernel, dim3((unsigned)((cwords + 255) / 256)), dim3(256), 0, s, rows, d_init.p, nlist, words, d_cent.p);
  ZCHK(hipGetLastError());
  ZRET(w.set_centroids(d_cent, nlist, s));
  ZCHK(hipStreamSynchronize(s));         // (`init` is a local)
  // 2. - 4. label, count bits per list, take the majority; a centroid without members keeps its bits
  const int cus = device_cus(c);
  for (uint32_t it = 0; it < iters; ++it) {
    ZRET(bivf_label(h, c, d_rows, n, d_labels, s));
    ZCHK(hipMemsetAsync(d_ones, 0, (size_t)nlist * dim * 4, s));
    ZCHK(hipMemsetAsync(d_members, 0, (size_t)nlist * 4, s));
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 3) / 4, (uint64_t)cus * 32);
    hipLaunchKernelGGL(bivf_bit_count_kernel, dim3(grid), dim3(256), 0, s, rows, d_labels.p, n, words, d_ones.p, d_members.p);
    hipLaunchKernelGGL(bivf_majority_kernel, dim3((unsigned)((cwords + 255) / 256)), dim3(256), 0, s, d_ones.p, d_members.p, nlist, words,
                       d_cent.p);
    ZCHK(hipGetLastError());
    ZRET(launch_pack(h->cent, d_cent, nlist, nullptr, 0, nullptr, s, h->cent.keys, nullptr));
  }
  // 5. the final labels; 6. a stable counting sort by label: inside a list the rows are in ascending original row number
  ZRET(bivf_label(h, c, d_rows, n, d_labels, s));
  std::vector<uint32_t> labels(n);
  h->h_cent.resize(cwords);
  ZCHK(hipMemcpyAsync(labels.data(), d_labels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipMemcpyAsync(h->h_cent.data(), d_cent, (size_t)cwords * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipStreamSynchronize(s));
  std::vector<uint64_t> off(nlist + 1, 0), perm(n), pkeys(n);
  for (uint64_t i = 0; i < n; ++i) {
    if (labels[i] >= nlist) return ZVEC_HIP_ERR_RUNTIME;
    ++off[labels[i] + 1];
  }
  for (uint32_t l = 0; l < nlist; ++l) off[l + 1] += off[l];
  {
    std::vector<uint64_t> cur(off.begin(), off.end() - 1);
    for (uint64_t i = 0; i < n; ++i) perm[cur[labels[i]]++] = i;
  }
  for (uint64_t p = 0; p < n; ++p) pkeys[p] = keys ? keys[perm[p]] : perm[p];
  ZRET(w.set_offsets(off, s));
  w.clear_rows();
  ZRET(h->lists.reserve(n, s));
  Scoped<uint64_t> d_perm, d_pkeys;
  ZRET(d_perm.alloc(n));
  ZRET(d_pkeys.alloc(n));
  ZCHK(hipMemcpyAsync(d_perm, perm.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  ZCHK(hipMemcpyAsync(d_pkeys, pkeys.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  ZRET(launch_pack(h->lists, d_rows, n, d_perm, 0, nullptr, s, h->lists.keys, d_pkeys));
  h->lists.n = n;
  ZCHK(hipStreamSynchronize(s));         // (the tables are locals)
  h->h_row_ids = std::move(perm);
  if (perm_out) *perm_out = std::move(d_perm);
  return 0;
}

static int bivf_build_args(zvec_hip_bivf_t h, const void *rows, uint64_t n, uint32_t nlist) {
  if (!h || !rows || n == 0 || nlist == 0 || nlist > n) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return n >= 0xfffffff0ull ? ZVEC_HIP_ERR_OUT_OF_RANGE : 0;
}

int zvec_hip_bivf_build_dev(zvec_hip_bivf_t h, const void *d_rows, uint64_t n, const uint64_t *keys, uint32_t nlist, uint32_t kmeans_iters,
                            uint64_t seed, void *stream) {
  ZRET(bivf_build_args(h, d_rows, n, nlist));
  ZCHK(hipSetDevice(h->device));
  BivfWrite w(h);
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : h->defctx->own;
  return w.done(bivf_build_locked(w, d_rows, n, keys, nlist, kmeans_iters, seed, s), s);
}

int zvec_hip_bivf_build(zvec_hip_bivf_t h, const void *rows, uint64_t n, const uint64_t *keys, uint32_t nlist, uint32_t kmeans_iters,
                        uint64_t seed) {
  ZRET(bivf_build_args(h, rows, n, nlist));
  ZCHK(hipSetDevice(h->device));
  BivfWrite w(h);
  hipStream_t s = h->defctx->own;
  Scoped<char> d_rows;
  auto body = [&]() -> int {
    const size_t bytes = (size_t)n * h->lists.row_bytes();
    ZRET(d_rows.alloc(bytes));
    ZCHK(hipMemcpyAsync(d_rows, rows, bytes, hipMemcpyHostToDevice, s));
    return bivf_build_locked(w, d_rows, n, keys, nlist, kmeans_iters, seed, s);
  };
  return w.done(body(), s);              // (synchronises before d_rows goes)
}

int zvec_hip_bivf_info(zvec_hip_bivf_t h, uint64_t *count, uint32_t *nlist) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (count) *count = h->loaded ? h->count : 0;
  if (nlist) *nlist = h->loaded ? h->nlist : 0;
  return 0;
}

int zvec_hip_bivf_export(zvec_hip_bivf_t h, void *centroids, uint64_t *list_offsets, uint64_t *row_ids) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (centroids) memcpy(centroids, h->h_cent.data(), h->h_cent.size() * 4);
  if (list_offsets) memcpy(list_offsets, h->h_off.data(), h->h_off.size() * 8);
  if (row_ids) {
    if (h->h_row_ids.empty())
      for (uint64_t p = 0; p < h->count; ++p) row_ids[p] = p;
    else
      memcpy(row_ids, h->h_row_ids.data(), h->h_row_ids.size() * 8);
  }
  return 0;
}

int zvec_hip_bivf_get_vectors(zvec_hip_bivf_t h, const uint64_t *list_positions, uint64_t n, void *out) {
  if (!h || (n && (!list_positions || !out))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0x7fffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  std::lock_guard<std::mutex> g(h->mu);
  std::lock_guard<std::mutex> gc(h->defctx->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  std::vector<uint64_t> pos(list_positions, list_positions + n);
  for (uint64_t p : pos)
    if (p >= h->count) return ZVEC_HIP_ERR_NO_EXIST;
  ZCHK(hipSetDevice(h->device));
  return store_get_rows(h->defctx, h->lists, pos, out);
}

// How a batch is cut: the tile runs per list and the queries per slice.  A list is cut into up to `nsplit` runs of tiles so that a
// small batch still fills the machine (about 16 one-wave work-groups per CU, as the flat Hamming scan), never more runs than the
// longest list has tiles; the partial lists of a slice — np * nsplit lists of k (score, position) pairs per query — stay within
// the byte cap, the centroid distances of a slice within dense_sub_batch's 1 GiB, and its query matrix below 2^32 chunks (the list
// scan addresses a query's first chunk with 32 bits).
struct BivfSlices {
  uint32_t nsplit = 1, slice = 1;
};
static BivfSlices bivf_slices(uint32_t count, uint32_t np, uint32_t topk, uint32_t max_tiles, uint32_t nlist, uint32_t cpr, int cus, uint64_t cap) {
  BivfSlices b;
  const uint64_t pairs = (uint64_t)count * np;
  b.nsplit = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(max_tiles, ((uint64_t)cus * 16 + pairs - 1) / pairs));
  const uint64_t per_list = (uint64_t)np * topk * 8;
  while (b.nsplit > 1 && per_list * b.nsplit > cap) b.nsplit /= 2;
  b.slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, cap / (per_list * b.nsplit)));
  b.slice = std::min(b.slice, dense_sub_batch(count, ((uint64_t)nlist + TILE_N - 1) / TILE_N * TILE_N));
  b.slice = std::min(b.slice, 0xffffffffu / cpr);
  return b;
}

// Stage 2 of zvec_hip_bivf_search_fp32: what the caller asked for, while the search proper runs with topk = kc and no radius.  The
// outputs of the search proper are then the caller's, [count][topk] long.
struct BivfRerank {
  const float *d_queries;       // [count][dim] fp32
  uint32_t dim, topk;
  float threshold;
};

// the candidate arrays of a re-ranked search inside c->bivf_cand: the scratch keys of one slice in front (8-byte aligned)
struct BivfCand {
  uint64_t *keys;
  uint32_t *pos;
  float *scores;
  uint32_t *counts;
};
static BivfCand bivf_cand_arrays(const zvec_hip_ctx_s *c, uint32_t count, uint32_t kc, uint32_t slice) {
  BivfCand b;
  b.keys = c->bivf_cand.as<uint64_t>();
  b.pos = reinterpret_cast<uint32_t *>(b.keys + (size_t)slice * kc);
  b.scores = reinterpret_cast<float *>(b.pos + (size_t)count * kc);
  b.counts = reinterpret_cast<uint32_t *>(b.scores + (size_t)count * kc);
  return b;
}

// the search proper; the caller holds c->mu and h->rw (shared) and has validated the arguments.  rr: the merge of every slice keeps
// list-order positions and Hamming scores in the context, and bivf_rerank_kernel writes the slice's outputs from them.
static int bivf_search_dev_locked(zvec_hip_bivf_s *h, zvec_hip_ctx_s *c, const void *d_queries, uint32_t count, uint32_t topk,
                                  float threshold, uint32_t nprobe, uint32_t max_scan_count, const uint64_t *d_exclude,
                                  uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, hipStream_t s,
                                  const BivfRerank *rr = nullptr) {
  const StoreView &st = h->lists;
  const uint32_t nlist = h->nlist, np = std::min(nprobe, nlist);
  c->sh.count = 0;              // (no certify step is pending, no flat route and no fp IVF plan to read back)
  c->route = 0;
  c->ivf_plan.route = 0;
  c->bivf_count = 0;
  c->bivf_cand_count = 0;
  const int cus = device_cus(c);
  const BivfSlices cutq = bivf_slices(count, np, topk, h->max_tiles, nlist, st.bin_chunks(), cus, (uint64_t)ropts().bivf_part_bytes.load(std::memory_order_relaxed));
  const uint32_t nsplit = cutq.nsplit;
  if ((uint64_t)cutq.slice * np * nsplit >= 0xffffffffull) return ZVEC_HIP_ERR_UNSUPPORTED;       // (slots are 32-bit)
  ZRET(c->bivf_probe.ensure(((size_t)count * np + 2 * (size_t)count) * sizeof(uint32_t)));
  uint32_t *pidx = c->bivf_probe.as<uint32_t>(), *pcnt = pidx + (size_t)count * np, *pscan = pcnt + count;
  BivfCand cand{};
  if (rr) {
    ZRET(c->bivf_cand.ensure((size_t)cutq.slice * topk * 8 + (size_t)count * topk * 8 + (size_t)count * 4));
    cand = bivf_cand_arrays(c, count, topk, cutq.slice);
  }
  for (uint32_t q0 = 0; q0 < count; q0 += cutq.slice) {
    const uint32_t m = std::min(cutq.slice, count - q0);
    const uint64_t pairs = (uint64_t)m * np;
    ZRET(prep_queries(c, st, static_cast<const char *>(d_queries) + (size_t)q0 * st.row_bytes(), m, threshold, s));
    // probe set: exact centroid distances, then the np smallest by (distance, index) and the max-scan rule
    BivfSelectArgs sel{};
    ZRET(bivf_centroid_scores(h, c, m, s, &sel.dump, &sel.dump_stride));
    // plan arrays of the slice: list_count | list_fill | list_items | list_qoff | item_off | csr_q | csr_slot
    ZRET(c->bivf_plan.ensure(((size_t)5 * nlist + 2 + 2 * pairs) * sizeof(uint32_t)));
    uint32_t *list_count = c->bivf_plan.as<uint32_t>(), *list_fill = list_count + nlist, *list_items = list_fill + nlist,
             *list_qoff = list_items + nlist, *item_off = list_qoff + nlist + 1, *csr_q = item_off + nlist + 1, *csr_slot = csr_q + pairs;
    ZCHK(hipMemsetAsync(list_count, 0, (size_t)2 * nlist * sizeof(uint32_t), s));
    sel.nq = m; sel.nlist = nlist; sel.np = np; sel.max_scan_count = max_scan_count; sel.list_off = h->d_off;
    sel.probe_idx = pidx + (size_t)q0 * np; sel.probe_cnt = pcnt + q0; sel.scanned = pscan + q0; sel.list_count = list_count;
    hipLaunchKernelGGL(bivf_probe_select_kernel, dim3((m + 3) / 4), dim3(256), 0, s, sel);
    BivfPlanArgs p{};
    p.probe_idx = sel.probe_idx; p.probe_cnt = sel.probe_cnt; p.nq = m; p.np = np; p.nlist = nlist; p.nsplit = nsplit;
    p.list_off = h->d_off; p.list_count = list_count; p.list_items = list_items; p.list_fill = list_fill; p.list_qoff = list_qoff;
    p.csr_q = csr_q; p.csr_slot = csr_slot;
    hipLaunchKernelGGL(u32_exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, list_count, list_qoff, nlist, list_qoff + nlist);
    hipLaunchKernelGGL(bivf_plan_items_kernel, dim3((nlist + 255) / 256), dim3(256), 0, s, p);
    hipLaunchKernelGGL(u32_exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, list_items, item_off, nlist, item_off + nlist);
    hipLaunchKernelGGL(bivf_plan_scatter_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, p);
    ZCHK(hipGetLastError());
    // partial lists [m][np * nsplit][k]; the slots no item writes hold +inf / IDX_NONE
    const uint64_t entries = pairs * nsplit * topk;
    ZRET(c->part_s.ensure(entries * sizeof(float)));
    ZRET(c->part_i.ensure(entries * sizeof(uint32_t)));
    hipLaunchKernelGGL(bivf_fill_partials_kernel, dim3((unsigned)std::min<uint64_t>((entries + 255) / 256, (uint64_t)cus * 8)), dim3(256), 0, s,
                       c->part_s.as<float>(), c->part_i.as<uint32_t>(), entries);
    HamListScanArgs a{};
    a.base = reinterpret_cast<const uint32_t *>(st.base); a.exclude = reinterpret_cast<const uint32_t *>(d_exclude);
    a.queries = c->qpad.as<uint32_t>(); a.cpr = st.bin_chunks(); a.k = topk; a.threshold = threshold; a.nlist = nlist; a.nsplit = nsplit;
    a.list_off = h->d_off; a.list_qoff = list_qoff; a.item_off = item_off; a.csr_q = csr_q; a.csr_slot = csr_slot;
    a.gtau = c->gtau.as<uint32_t>(); a.part_s = c->part_s.as<float>(); a.part_i = c->part_i.as<uint32_t>();
    // an upper bound of the items: a probed list has at most count / 32 + 1 query blocks, each over at most nsplit tile runs
    const uint64_t bound = (pairs / HAM_QB + std::min<uint64_t>(nlist, pairs)) * nsplit;
    if (bound > 0x7fffffffull) return ZVEC_HIP_ERR_UNSUPPORTED;
    if (a.exclude) hipLaunchKernelGGL(hamming_list_scan_kernel<true>, dim3((unsigned)bound), dim3(64), ham_lds_bytes(topk), s, a);
    else hipLaunchKernelGGL(hamming_list_scan_kernel<false>, dim3((unsigned)bound), dim3(64), ham_lds_bytes(topk), s, a);
    ZCHK(hipGetLastError());
    if (!rr) {
      const SearchOut out{d_out_keys + (size_t)q0 * topk, d_out_scores + (size_t)q0 * topk, nullptr, d_out_counts + q0};
      ZRET(launch_merge(merge_partials(a.part_s, a.part_i, np * nsplit, a.gtau, topk, threshold, st.keys, out), m, merge_threads(m), s));
      continue;
    }
    // stage 1 ends as positions (the merge's key column is scratch), stage 2 re-scores them on the fp32 rows
    const SearchOut out{cand.keys, cand.scores + (size_t)q0 * topk, cand.pos + (size_t)q0 * topk, cand.counts + q0};
    ZRET(launch_merge(merge_partials(a.part_s, a.part_i, np * nsplit, a.gtau, topk, threshold, nullptr, out), m, merge_threads(m), s));
    BivfRerankArgs r{};
    r.rows = h->frows; r.queries = rr->d_queries + (size_t)q0 * rr->dim; r.cand = out.idx; r.cand_cnt = out.counts; r.keymap = st.keys;
    r.dim = rr->dim; r.kc = topk; r.topk = rr->topk; r.ip = h->fmetric == ZVEC_HIP_METRIC_IP ? 1u : 0u;
    r.threshold = std::min(rr->threshold, FLT_MAX);
    r.out_keys = d_out_keys + (size_t)q0 * rr->topk; r.out_scores = d_out_scores + (size_t)q0 * rr->topk; r.out_counts = d_out_counts + q0;
    hipLaunchKernelGGL(bivf_rerank_kernel, dim3(m), dim3(256), bivf_rerank_lds_bytes(rr->dim), s, r);
    ZCHK(hipGetLastError());
  }
  c->bivf_owner = h;
  c->bivf_count = count;
  c->bivf_np = np;
  if (rr) {
    c->bivf_cand_count = count;
    c->bivf_cand_kc = topk;
    c->bivf_cand_slice = cutq.slice;
  }
  return 0;
}

static int bivf_search_args(zvec_hip_bivf_t h, const void *queries, uint32_t count, uint32_t topk, uint32_t nprobe, const void *keys,
                            const void *scores, const void *counts) {
  if (!h || !queries || !keys || !scores || !counts) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count && (topk == 0 || nprobe == 0)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return topk > HAM_FUSED_MAX_K ? ZVEC_HIP_ERR_UNSUPPORTED : 0;       // (the dense-score route of long lists is not built here)
}

int zvec_hip_bivf_search_dev(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk, float threshold,
                             uint32_t nprobe, uint32_t max_scan_count, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                             float *d_out_scores, uint32_t *d_out_counts, void *stream) {
  ZRET(bivf_search_args(h, d_queries, count, topk, nprobe, d_out_keys, d_out_scores, d_out_counts));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  ZCHK(hipSetDevice(h->device));
  return bivf_search_dev_locked(h, c, d_queries, count, topk, threshold, nprobe, max_scan_count, d_exclude_bitset, d_out_keys, d_out_scores,
                                d_out_counts, pick_stream(c, stream));
}

int zvec_hip_bivf_search(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count, uint32_t topk, float threshold,
                         uint32_t nprobe, uint32_t max_scan_count, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts) {
  ZRET(bivf_search_args(h, queries, count, topk, nprobe, out_keys, out_scores, out_counts));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);                // ONE critical section from the upload to the copy-out (zvec_hip_flat_search)
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw);        // the row count the bitset is sized for == the rows of the lists
    if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
    ZRET(host_search_wrap_begin(c, queries, (size_t)count * h->lists.row_bytes(), exclude_bitset, h->count, count, topk, c->cur));
    ZRET(bivf_search_dev_locked(h, c, c->io_qp, count, topk, threshold, nprobe, max_scan_count,
                                exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr, c->io_keys.as<uint64_t>(), c->io_scores.as<float>(),
                                c->io_counts.as<uint32_t>(), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

int zvec_hip_bivf_last_probes(zvec_hip_bivf_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t *probe_idx, uint32_t *probe_cnt,
                              uint32_t *scanned) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->bivf_owner != h || c->bivf_count == 0 || count > c->bivf_count) return ZVEC_HIP_ERR_NO_READY;
  ZCHK(hipSetDevice(h->device));
  ZCHK(hipStreamSynchronize(c->cur));
  const uint32_t *pidx = c->bivf_probe.as<uint32_t>(), *pcnt = pidx + (size_t)c->bivf_count * c->bivf_np, *pscan = pcnt + c->bivf_count;
  if (probe_idx) ZCHK(hipMemcpy(probe_idx, pidx, (size_t)count * c->bivf_np * 4, hipMemcpyDeviceToHost));
  if (probe_cnt) ZCHK(hipMemcpy(probe_cnt, pcnt, (size_t)count * 4, hipMemcpyDeviceToHost));
  if (scanned) ZCHK(hipMemcpy(scanned, pscan, (size_t)count * 4, hipMemcpyDeviceToHost));
  return 0;
}
