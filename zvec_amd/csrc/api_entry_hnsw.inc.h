// api_entry_hnsw.inc.h — C ABI entry points: batched k-NN search on a built HNSW graph (zvec_hip_hnsw_*; inside extern "C").
// Device code: zvk_hnsw.hip.h.  A handle family of its own beside the flat and IVF handles: it loads a graph somebody else built
// and walks it by the rule of DESIGN §3c (HnswAlgorithm::search, hnsw_algorithm.cc:83-278).  api_entry_hnsw_build.inc.h builds one.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// dst: a block of new_count elements whose first old_count are src's (device to device) and whose others are `fill` bytes; the work
// is queued on `s`, in order with the kernels that follow on it
extern "C++" template <typename T>
static int hnsw_regrow(Scoped<T> &dst, const Scoped<T> &src, size_t old_count, size_t new_count, int fill, hipStream_t s) {
  ZRET(dst.alloc(std::max<size_t>(new_count, 1)));
  if (old_count) ZCHK(hipMemcpyAsync(dst.p, src.p, old_count * sizeof(T), hipMemcpyDeviceToDevice, s));
  if (new_count > old_count) ZCHK(hipMemsetAsync(dst.p + old_count, fill, (new_count - old_count) * sizeof(T), s));
  return 0;
}

// A graph on the device: its numbers (HnswShape, host/hnsw_add_plan.h) and its arrays, everything a load or a build replaces whole
// and an add grows.  Behind n / n_upper the rows, lists and counts are zero and upper_of is IDX_NONE.  Every size below comes from
// the shape; rows are stored pad_bytes apart.
struct HnswGraph : HnswShape {
  struct Arrays {
    Scoped<unsigned char> rows;        // [cap_rows][dpad] elements
    Scoped<uint64_t> keys;             // [cap_rows]
    Scoped<uint32_t> nbr0, cnt0, upper_of, nbr_up, cnt_up;      // [cap_rows] each per row; the upper two [cap_upper][stride]
  } arr;

  // Room for to.cap_rows rows and, under the stride to.stride (0: no upper lists, nothing is made), to.cap_upper nodes of level >= 1
  // with lists of to.m0 / to.m; writes those five numbers and no other.  Never shrinks; what is not too small stays where it is.
  // Old slot (u, l) of the upper table goes to new slot (u, l).  Every new block is allocated before the graph changes.  The caller
  // holds the handle exclusively and has synchronised the device.
  int resize(const HnswShape &to, size_t pad_bytes, hipStream_t s, bool &grew_rows, bool &grew_upper) {
    const size_t old_stride = stride, old_upper = n_upper;
    const uint64_t rows_to = std::max(to.cap_rows, cap_rows), upper_to = to.stride ? std::max(to.cap_upper, cap_upper) : 0;
    grew_rows = rows_to > cap_rows;
    grew_upper = to.stride && upper_to > cap_upper;
    const bool make_upper_of = to.stride && !old_stride;
    const bool move_table = to.stride && (to.stride != old_stride || grew_upper);
    Arrays g;
    if (grew_rows) {
      ZRET(hnsw_regrow(g.rows, arr.rows, (size_t)n * pad_bytes, (size_t)rows_to * pad_bytes, 0, s));
      ZRET(hnsw_regrow(g.keys, arr.keys, (size_t)n, (size_t)rows_to, 0, s));
      ZRET(hnsw_regrow(g.cnt0, arr.cnt0, (size_t)n, (size_t)rows_to, 0, s));
      ZRET(hnsw_regrow(g.nbr0, arr.nbr0, (size_t)n * to.m0, (size_t)rows_to * to.m0, 0, s));
    }
    if (to.stride && (grew_rows || make_upper_of)) ZRET(hnsw_regrow(g.upper_of, arr.upper_of, old_stride ? (size_t)n : 0, (size_t)rows_to, 0xff, s));
    if (move_table) {
      const size_t slots = (size_t)upper_to * to.stride;
      const bool same = to.stride == old_stride;
      ZRET(hnsw_regrow(g.cnt_up, arr.cnt_up, same ? old_upper * old_stride : 0, slots, 0, s));
      ZRET(hnsw_regrow(g.nbr_up, arr.nbr_up, same ? old_upper * old_stride * to.m : 0, slots * to.m, 0, s));
      if (!same && old_stride && old_upper) {
        const uint64_t threads = (uint64_t)old_upper * old_stride * std::max(to.m, 1u);
        hipLaunchKernelGGL(hnsw_restride_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, arr.nbr_up.p, arr.cnt_up.p,
                           g.nbr_up.p, g.cnt_up.p, (uint64_t)old_upper, (uint32_t)old_stride, to.stride, to.m);
        ZCHK(hipGetLastError());
      }
    }
    ZCHK(hipStreamSynchronize(s));               // (the copies have read the old blocks, the new ones are whole)
    if (g.rows.p) { std::swap(arr.rows, g.rows); std::swap(arr.keys, g.keys); std::swap(arr.cnt0, g.cnt0); std::swap(arr.nbr0, g.nbr0); }
    if (g.upper_of.p) std::swap(arr.upper_of, g.upper_of);
    if (g.cnt_up.p) { std::swap(arr.cnt_up, g.cnt_up); std::swap(arr.nbr_up, g.nbr_up); }
    cap_rows = rows_to; m0 = to.m0;              // the old blocks go with the local
    if (to.stride) { cap_upper = upper_to; stride = to.stride; m = to.m; }
    return 0;
  }

  // count rows of row_bytes (on the device or on the host) to the places first .. first + count - 1, the padding of each zeroed;
  // and their keys, or their positions when keys is NULL
  int put_rows(uint64_t first, uint64_t count, const void *rows, bool on_device, const uint64_t *keys, size_t row_bytes, size_t pad_bytes) {
    if (count == 0) return 0;
    unsigned char *dst = arr.rows.p + (size_t)first * pad_bytes;
    if (pad_bytes != row_bytes) ZCHK(hipMemset(dst, 0, (size_t)count * pad_bytes));
    ZCHK(hipMemcpy2D(dst, pad_bytes, rows, row_bytes, row_bytes, count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    std::vector<uint64_t> id;
    if (!keys) {
      id.resize(count);
      for (uint64_t i = 0; i < count; ++i) id[i] = first + i;
      keys = id.data();
    }
    ZCHK(hipMemcpy(arr.keys.p + first, keys, (size_t)count * 8, hipMemcpyHostToDevice));
    return 0;
  }

  // the graph as the kernels read it; the caller adds what its walk needs
  HnswArgs args(uint32_t dim, uint32_t dpad, int metric) const {
    HnswArgs a{};
    a.rows = arr.rows; a.keys = arr.keys; a.nbr0 = arr.nbr0; a.cnt0 = arr.cnt0; a.upper_of = arr.upper_of;
    a.nbr_up = arr.nbr_up; a.cnt_up = arr.cnt_up;
    a.n = (uint32_t)n; a.dim = dim; a.dpad = dpad; a.m0 = m0; a.m = m; a.max_level = stride; a.entry = entry;
    a.ip = metric == ZVEC_HIP_METRIC_IP ? 1 : 0;
    return a;
  }
};

// What one insertion did: hnsw_insert_apply (api_entry_hnsw_build.inc.h) fills it, zvec_hip_hnsw_last_build_info and _last_add_info
// hand it out.
struct HnswInsertDone {
  uint32_t rounds = 0, slices = 0, one = 0;      // slices: the most of a round's insert phase; one: rounds on the one-node path
  uint32_t top = 0, entry = 0;                   // after the call
  double insert_ms = 0, reverse_ms = 0;
  uint64_t dists = 0, requests = 0, prunes = 0;
  uint64_t first = 0, count = 0, cap_rows = 0, cap_upper = 0;
  bool grew_rows = false, grew_upper = false, restrided = false;
};

struct zvec_hip_hnsw_s {
  int device = 0;
  int metric = 0;
  int dtype = ZVEC_HIP_DT_FP32;        // of rows and queries: fp32, or fp16 (zvec_hip_hnsw_create_typed); halves are stored as halves
  uint32_t esz = 4;                    // bytes per element
  uint32_t dim = 0, dpad = 0;          // dpad: elements per stored row, dim rounded up to 4 (a lane of the kernel loads four elements)
  bool loaded = false;
  HnswGraph graph;                     // n and n_upper after a load or a build have exactly their room; an add or a reserve makes more
  uint64_t want_rows = 0, want_upper = 0;        // what zvec_hip_hnsw_reserve asked for: the least an add grows to
  zvec_hip_hnsw_build_params params{};           // of the last build (an add on a handle without nodes is one); all zero after a load
  bool built = false;                  // bdone is the last build's
  HnswInsertDone bdone;
  bool added = false;                  // adone is the last add's
  HnswInsertDone adone;
  zvec_hip_ctx_s *defctx = nullptr;
  // Lock order: mu, a context's mutex, rw.  A writer (HnswWrite) holds mu, defctx's mutex and rw exclusively; a search holds the
  // mutex of the context it works through, then rw shared (as zvec_hip_flat_s); info, export and get_vectors hold rw shared alone.
  std::mutex mu;                       // serialises the calls that change the index or use defctx's workspace
  FairSharedMutex rw;
  bool f16() const { return dtype == ZVEC_HIP_DT_FP16; }
  size_t row_bytes() const { return (size_t)dim * esz; }           // of a row as callers pass it
  size_t pad_bytes() const { return (size_t)dpad * esz; }          // of a row as it is stored
  ~zvec_hip_hnsw_s() { delete defctx; }
};

// the instantiation of a kernel template for the handle's element type
#define HNSW_KERNEL(h, k) ((h)->f16() ? k<true> : k<false>)

// One change of an HNSW handle (IvfWrite's twin): h->mu, the built-in context's mutex (the rounds use its stream and workspace) and
// h->rw exclusively, in the handle's lock order, while it lives.
struct HnswWrite {
  zvec_hip_hnsw_s *const h;
  explicit HnswWrite(zvec_hip_hnsw_s *h_) : h(h_), g(h_->mu), gc(h_->defctx->mu), w(h_->rw) {}
  int open() { ZCHK(hipSetDevice(h->device)); return 0; }
  // before the first touch of the arrays: searches enqueued on other contexts have finished with them
  int quiesce() { ZCHK(hipDeviceSynchronize()); return 0; }

 private:
  std::lock_guard<std::mutex> g, gc;
  std::unique_lock<FairSharedMutex> w;
};

// The one place a graph becomes the handle's: g is h->graph itself (an add in place) or a fresh one that takes its place, the old
// arrays going with `g`.  The shape is normalised here and nowhere else (hnsw_shape_kept).
static void hnsw_commit(zvec_hip_hnsw_s *h, HnswGraph &g) {
  if (&g != &h->graph) std::swap(h->graph, g);
  static_cast<HnswShape &>(h->graph) = hnsw_shape_kept(h->graph);
  h->loaded = true;
  h->defctx->hnsw_count = 0;
}

int zvec_hip_hnsw_create_typed(uint32_t dim, int dtype, int metric, int device, zvec_hip_hnsw_t *out) {
  if (!out || dim == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype != ZVEC_HIP_DT_FP32 && dtype != ZVEC_HIP_DT_FP16) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (metric != ZVEC_HIP_METRIC_L2 && metric != ZVEC_HIP_METRIC_IP) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (dim > HNSW_MAX_DIM) return ZVEC_HIP_ERR_UNSUPPORTED;          // (the query row is kept in LDS)
  zvec_hip_ctx_s *c = nullptr;
  ZRET(ctx_new(device, &c));
  zvec_hip_hnsw_s *h = new (std::nothrow) zvec_hip_hnsw_s();
  if (!h) { ctx_free(c); return ZVEC_HIP_ERR_NO_MEMORY; }
  h->device = device; h->metric = metric; h->dim = dim; h->dpad = (dim + 3) / 4 * 4; h->defctx = c;
  h->dtype = dtype; h->esz = dtype == ZVEC_HIP_DT_FP16 ? 2 : 4;
  *out = h;
  return 0;
}

// the fp32 creator: every other type stays Unsupported here, fp16 included (zvec_hip_hnsw_create_typed takes it)
int zvec_hip_hnsw_create(uint32_t dim, int dtype, int metric, int device, zvec_hip_hnsw_t *out) {
  if (!out || dim == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype != ZVEC_HIP_DT_FP32) return ZVEC_HIP_ERR_UNSUPPORTED;
  return zvec_hip_hnsw_create_typed(dim, dtype, metric, device, out);
}

int zvec_hip_hnsw_dtype(zvec_hip_hnsw_t h, int *dtype) {
  if (!h || !dtype) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  *dtype = h->dtype;
  return 0;
}

int zvec_hip_hnsw_destroy(zvec_hip_hnsw_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
  return 0;
}

// what zvec_hip_hnsw_load refuses before it touches the handle
static int hnsw_validate(uint64_t n, const void *rows, uint32_t m0, const uint32_t *nbr0, const uint32_t *cnt0, uint32_t max_level,
                         uint32_t m, uint32_t n_upper, const uint32_t *upper_of, const uint32_t *nbr_up, const uint32_t *cnt_up,
                         uint32_t entry_point) {
  if (n == 0) return 0;
  if (n >= 0xfffffff0ull) return ZVEC_HIP_ERR_OUT_OF_RANGE;         // node ids are 32-bit (IDX_NONE reserved)
  if (!rows || !cnt0 || (m0 && !nbr0) || entry_point >= n) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const bool up = max_level >= 1;
  if (up && (!upper_of || n_upper == 0 || !cnt_up || (m && !nbr_up) || n_upper > n)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  for (uint64_t i = 0; i < n; ++i) {
    if (cnt0[i] > m0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    for (uint32_t j = 0; j < cnt0[i]; ++j)
      if (nbr0[i * m0 + j] >= n) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    if (up && upper_of[i] != IDX_NONE && upper_of[i] >= n_upper) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  }
  if (!up) return 0;
  if (upper_of[entry_point] == IDX_NONE) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  for (uint64_t s = 0; s < (uint64_t)n_upper * max_level; ++s) {
    if (cnt_up[s] > m) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    for (uint32_t j = 0; j < cnt_up[s]; ++j) {
      const uint32_t v = nbr_up[s * m + j];
      // (the walk reads the upper lists of every node it moves to: a neighbour on an upper level has them)
      if (v >= n || upper_of[v] == IDX_NONE) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    }
  }
  return 0;
}

// HnswSearcher::load (hnsw_searcher.cc) in the shape of plain arrays: the graph as HnswEntity serves it to the algorithm
// (get_neighbors(level, id), get_vector(id), get_key(id), entry_point(), cur_max_level())
int zvec_hip_hnsw_load(zvec_hip_hnsw_t h, uint64_t n, const void *rows, const uint64_t *keys, uint32_t m0, const uint32_t *nbr0,
                       const uint32_t *cnt0, uint32_t max_level, uint32_t m, uint32_t n_upper, const uint32_t *upper_of,
                       const uint32_t *nbr_up, const uint32_t *cnt_up, uint32_t entry_point) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZRET(hnsw_validate(n, rows, m0, nbr0, cnt0, max_level, m, n_upper, upper_of, nbr_up, cnt_up, entry_point));
  HnswWrite w(h);
  ZRET(w.open());
  ZRET(w.quiesce());
  HnswGraph g;                                   // a fresh graph with exactly the room of the caller's
  HnswShape to;
  to.n = to.cap_rows = n; to.m0 = m0; to.m = m; to.stride = max_level; to.n_upper = n_upper; to.cap_upper = n_upper; to.entry = entry_point;
  if (n) {
    bool grew_rows, grew_upper;
    ZRET(g.resize(to, h->pad_bytes(), h->defctx->cur, grew_rows, grew_upper));
    ZRET(g.put_rows(0, n, rows, false, keys, h->row_bytes(), h->pad_bytes()));
    const size_t slots = (size_t)n_upper * max_level;
    ZCHK(hipMemcpy(g.arr.cnt0, cnt0, (size_t)n * 4, hipMemcpyHostToDevice));
    if (m0) ZCHK(hipMemcpy(g.arr.nbr0, nbr0, (size_t)n * m0 * 4, hipMemcpyHostToDevice));
    if (max_level) {
      ZCHK(hipMemcpy(g.arr.upper_of, upper_of, (size_t)n * 4, hipMemcpyHostToDevice));
      ZCHK(hipMemcpy(g.arr.cnt_up, cnt_up, slots * 4, hipMemcpyHostToDevice));
      if (m) ZCHK(hipMemcpy(g.arr.nbr_up, nbr_up, slots * m * 4, hipMemcpyHostToDevice));
    }
  }
  static_cast<HnswShape &>(g) = to;
  hnsw_commit(h, g);                             // the old arrays go with the local
  h->params = zvec_hip_hnsw_build_params();
  return 0;
}

int zvec_hip_hnsw_info(zvec_hip_hnsw_t h, uint64_t *n, uint32_t *dim, uint32_t *m0, uint32_t *max_level, uint32_t *m, uint32_t *n_upper,
                       uint32_t *entry_point) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  const HnswShape &g = h->graph;
  if (n) *n = g.n;
  if (dim) *dim = h->dim;
  if (m0) *m0 = g.m0;
  if (max_level) *max_level = g.stride;
  if (m) *m = g.m;
  if (n_upper) *n_upper = g.n_upper;
  if (entry_point) *entry_point = g.entry;
  return 0;
}

int zvec_hip_hnsw_get_vectors(zvec_hip_hnsw_t h, const uint64_t *positions, uint64_t n, void *out) {
  if (!h || (n && (!positions || !out))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  for (uint64_t i = 0; i < n; ++i)
    if (positions[i] >= h->graph.n) return ZVEC_HIP_ERR_NO_EXIST;
  ZCHK(hipSetDevice(h->device));
  for (uint64_t i = 0; i < n; ++i)
    ZCHK(hipMemcpy(static_cast<unsigned char *>(out) + (size_t)i * h->row_bytes(), h->graph.arr.rows.p + (size_t)positions[i] * h->pad_bytes(),
                   h->row_bytes(), hipMemcpyDeviceToHost));
  return 0;
}

int zvec_hip_hnsw_export(zvec_hip_hnsw_t h, uint64_t *keys, uint32_t *nbr0, uint32_t *cnt0, uint32_t *upper_of, uint32_t *nbr_up,
                         uint32_t *cnt_up) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  const HnswGraph &g = h->graph;
  if (g.n == 0) return 0;
  ZCHK(hipSetDevice(h->device));
  const size_t n = g.n, slots = (size_t)g.n_upper * g.stride;
  if (keys) ZCHK(hipMemcpy(keys, g.arr.keys, n * 8, hipMemcpyDeviceToHost));
  if (nbr0 && g.m0) ZCHK(hipMemcpy(nbr0, g.arr.nbr0, n * g.m0 * 4, hipMemcpyDeviceToHost));
  if (cnt0) ZCHK(hipMemcpy(cnt0, g.arr.cnt0, n * 4, hipMemcpyDeviceToHost));
  if (g.stride == 0) return 0;
  if (upper_of) ZCHK(hipMemcpy(upper_of, g.arr.upper_of, n * 4, hipMemcpyDeviceToHost));
  if (nbr_up && g.m) ZCHK(hipMemcpy(nbr_up, g.arr.nbr_up, slots * g.m * 4, hipMemcpyDeviceToHost));
  if (cnt_up) ZCHK(hipMemcpy(cnt_up, g.arr.cnt_up, slots * 4, hipMemcpyDeviceToHost));
  return 0;
}

// The search proper; the caller holds c->mu and h->rw (shared) and has validated the arguments.  A batch goes in slices of queries so
// that the visited bits (ceil(n / 32) words per query) and the candidate regions (min(max_scan, n) words of 8 bytes per query, only
// when that is more than the kernel holds in LDS) stay within the "hnsw_ws_bytes" option; a query's walk does not depend on its slice.
static int hnsw_search_dev_locked(zvec_hip_hnsw_s *h, zvec_hip_ctx_s *c, const void *d_queries, uint32_t count, uint32_t topk, uint32_t ef,
                                  uint32_t max_scan, float threshold, const uint64_t *d_exclude, uint64_t *d_out_keys, float *d_out_scores,
                                  uint32_t *d_out_counts, hipStream_t s) {
  c->sh.count = 0;              // (no certify step is pending, no flat route and no IVF plan to read back)
  c->route = 0;
  c->ivf_plan.route = 0;
  c->hnsw_count = 0;
  ZRET(c->hnsw_stats.ensure((size_t)count * 8));
  uint32_t slices = 0;
  if (h->graph.n == 0) {
    hipLaunchKernelGGL(hnsw_empty_kernel, dim3((count * std::max(topk, 2u) + 255) / 256), dim3(256), 0, s, d_out_keys, d_out_scores,
                       d_out_counts, c->hnsw_stats.as<uint32_t>(), count, topk);
    ZCHK(hipGetLastError());
  } else {
    HnswArgs a = h->graph.args(h->dim, h->dpad, h->metric);
    const uint32_t n = a.n;
    a.exclude = reinterpret_cast<const uint32_t *>(d_exclude);
    a.topk = topk; a.ef = std::max(ef, topk); a.max_scan = max_scan ? max_scan : n; a.threshold = threshold;
    a.vis_words = (n + 31) / 32;
    a.ccap = std::min(a.max_scan, n);
    const bool spill = a.ccap > HNSW_C_LDS;
    const uint64_t per_q = (uint64_t)a.vis_words * 4 + (spill ? (uint64_t)a.ccap * 8 : 0);
    const uint64_t budget = (uint64_t)ropts().hnsw_ws_bytes.load(std::memory_order_relaxed);
    const uint32_t slice = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(count, budget / per_q));
    ZRET(c->hnsw_ws.ensure((size_t)slice * per_q));
    uint64_t *cand = spill ? c->hnsw_ws.as<uint64_t>() : nullptr;
    uint32_t *vis = reinterpret_cast<uint32_t *>(c->hnsw_ws.as<uint64_t>() + (spill ? (size_t)slice * a.ccap : 0));
    for (uint32_t q0 = 0; q0 < count; q0 += slice, ++slices) {
      const uint32_t mq = std::min(slice, count - q0);
      ZCHK(hipMemsetAsync(vis, 0, (size_t)mq * a.vis_words * 4, s));
      a.queries = static_cast<const unsigned char *>(d_queries) + (size_t)q0 * h->row_bytes();
      a.visited = vis; a.cand_ws = cand;
      a.out_keys = d_out_keys + (size_t)q0 * topk; a.out_scores = d_out_scores + (size_t)q0 * topk; a.out_counts = d_out_counts + q0;
      a.stats = c->hnsw_stats.as<uint32_t>() + 2 * (size_t)q0;
      hipLaunchKernelGGL(HNSW_KERNEL(h, hnsw_search_kernel), dim3(mq), dim3(64), hnsw_lds_bytes(a.dpad, a.ef), s, a);
      ZCHK(hipGetLastError());
    }
  }
  c->hnsw_owner = h;
  c->hnsw_count = count;
  c->hnsw_slices = slices;
  return 0;
}

static int hnsw_search_args(zvec_hip_hnsw_t h, const void *queries, uint32_t count, uint32_t topk, uint32_t ef, const void *keys,
                            const void *scores, const void *counts) {
  if (!h || !queries || !keys || !scores || !counts) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count && topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return std::max(ef, topk) > HNSW_MAX_EF ? ZVEC_HIP_ERR_UNSUPPORTED : 0;
}

// HnswSearcher::search_impl (hnsw_searcher.cc) above the brute-force hand-over, which stays with the caller
int zvec_hip_hnsw_search_dev(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count, uint32_t topk, uint32_t ef,
                             uint32_t max_scan, float threshold, const uint64_t *d_exclude_bitset, uint64_t *d_out_keys,
                             float *d_out_scores, uint32_t *d_out_counts, void *stream) {
  ZRET(hnsw_search_args(h, d_queries, count, topk, ef, d_out_keys, d_out_scores, d_out_counts));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  ZCHK(hipSetDevice(h->device));
  return hnsw_search_dev_locked(h, c, d_queries, count, topk, ef, max_scan, threshold, d_exclude_bitset, d_out_keys, d_out_scores,
                                d_out_counts, pick_stream(c, stream));
}

int zvec_hip_hnsw_search(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count, uint32_t topk, uint32_t ef,
                         uint32_t max_scan, float threshold, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts) {
  ZRET(hnsw_search_args(h, queries, count, topk, ef, out_keys, out_scores, out_counts));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);                // ONE critical section from the upload to the copy-out (zvec_hip_flat_search)
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw);        // the row count the bitset is sized for == the nodes of the graph
    if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
    ZRET(host_search_wrap_begin(c, queries, (size_t)count * h->row_bytes(), h->graph.n ? exclude_bitset : nullptr, h->graph.n, count, topk, c->cur));
    ZRET(hnsw_search_dev_locked(h, c, c->io_qp, count, topk, ef, max_scan, threshold,
                                exclude_bitset && h->graph.n ? c->io_ex.as<uint64_t>() : nullptr, c->io_keys.as<uint64_t>(),
                                c->io_scores.as<float>(), c->io_counts.as<uint32_t>(), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

int zvec_hip_hnsw_last_stats(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, uint32_t count, uint32_t *out_scanned, uint32_t *out_hops,
                             uint32_t *out_slices) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->hnsw_owner != h || c->hnsw_count == 0 || count > c->hnsw_count) return ZVEC_HIP_ERR_NO_READY;
  ZCHK(hipSetDevice(h->device));
  ZCHK(hipStreamSynchronize(c->cur));
  std::vector<uint32_t> st((size_t)count * 2);
  ZCHK(hipMemcpy(st.data(), c->hnsw_stats.p, st.size() * 4, hipMemcpyDeviceToHost));
  for (uint32_t q = 0; q < count; ++q) {
    if (out_scanned) out_scanned[q] = st[2 * (size_t)q];
    if (out_hops) out_hops[q] = st[2 * (size_t)q + 1];
  }
  if (out_slices) *out_slices = c->hnsw_slices;
  return 0;
}
