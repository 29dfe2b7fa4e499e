// api_types.inc.h — error macros, device buffers, the blocked Store, context and index handle structs
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

#define ZCHK(expr)                                                                               \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      fprintf(stderr, "[zvec_hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e),        \
              __FILE__, __LINE__);                                                               \
      return (_e == hipErrorOutOfMemory) ? ZVEC_HIP_ERR_NO_MEMORY : ZVEC_HIP_ERR_RUNTIME;        \
    }                                                                                            \
  } while (0)

#define ZRET(expr)            \
  do {                        \
    int _r = (expr);          \
    if (_r != 0) return _r;   \
  } while (0)

namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int PROFILE_MAX = 8192;

// The one place device memory is allocated and freed: a typed hipMalloc block that its destructor gives back.  Move-only (a move
// assignment hands the old block to the source, which frees it when it goes); as a local it is the device temporary of a function,
// freed on every exit path.
template <typename T>
struct Scoped {
  T *p = nullptr;
  size_t cap = 0;        // bytes
  Scoped() {}
  Scoped(Scoped &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Scoped &operator=(Scoped &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~Scoped() { release(); }
  int alloc_bytes(size_t bytes) {
    release();
    ZCHK(hipMalloc(reinterpret_cast<void **>(&p), bytes));
    cap = bytes;
    return 0;
  }
  int alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  operator T *() const { return p; }
};

// a host table as a device array of its own (a blocking copy)
template <typename T>
int upload(Scoped<T> &d, const T *src, size_t n) {
  ZRET(d.alloc(std::max<size_t>(n, 1)));
  ZCHK(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// workspace that grows on demand and keeps what it has grown to
struct DevBuf : Scoped<void> {
  int ensure(size_t bytes) { return bytes <= cap ? 0 : alloc_bytes(bytes + bytes / 4 + 256); }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// The hole bits of a flat or a sparse handle: add-with-id pads a gap in front of an id with rows under the invalid key that no search
// may return.  Host words (host/hole_bits.h) plus a device copy that every entry taking an exclude set ORs in while a hole exists
// (effective_exclude), reading its words for all of the store's rows.  So the protocol is reserve-first: whoever holds the handle's rw
// exclusively and is about to make the store `rows` long calls reserve() BEFORE the store changes — words and copy then span `rows`
// positions, new words zero; the copy grows through a block of its own, zeroed to its capacity, that receives the words as they are and
// takes the old one's place on success only —, sets and clears host bits while it stores, and ends with upload_dirty().  A handle TRACKS
// holes once a device copy exists, or the count is non-zero, or the call at hand leaves some (`leaves`): until then all of this is a no-op.
struct HoleBits {
  HoleWords host;
  uint64_t count() const { return host.nholes; }
  const uint64_t *device() const { return d_holes.as<uint64_t>(); }
  int reserve(uint64_t rows, bool leaves, hipStream_t s) {
    if (!leaves && count() == 0 && !d_holes.p) return 0;
    host.resize(rows);
    if (HoleWords::words_for(rows) * 8 <= d_holes.cap) return 0;
    DevBuf grown;
    ZRET(grown.ensure((size_t)HoleWords::words_for(rows) * 16));
    ZCHK(hipMemsetAsync(grown.p, 0, grown.cap, s));
    ZRET(upload(grown, 0, ~0ull, s));
    std::swap(d_holes, grown);                     // (the old block goes with the local: hipFree waits for the device)
    return 0;
  }
  int upload_dirty(hipStream_t s) {                // the words changed since the last upload reach the copy
    uint64_t lo, hi;
    return host.take_dirty(&lo, &hi) ? upload(d_holes, lo, hi, s) : 0;
  }

 private:
  DevBuf d_holes;
  int upload(DevBuf &to, uint64_t lo, uint64_t hi, hipStream_t s) {      // host words [lo, hi], as far as both sides have them
    const uint64_t have = std::min<uint64_t>(host.words.size(), to.cap / 8), end = hi < have ? hi + 1 : have;
    if (lo >= end) return 0;
    ZCHK(hipMemcpyAsync(to.as<uint64_t>() + lo, host.words.data() + lo, (size_t)(end - lo) * 8, hipMemcpyHostToDevice, s));
    ZCHK(hipStreamSynchronize(s));                 // (the words are pageable and may be resized by the next call)
    return 0;
  }
};

// a typed window into somebody else's device buffer
struct DevView {
  void *p = nullptr;
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// pinned host staging (small transfers of the host-pointer entry points: a copy from / to pageable memory is staged
// and synchronised by the runtime, a pinned one is a plain asynchronous DMA)
struct PinnedBuf {
  void *p = nullptr;
  void *dev = nullptr;   // the same bytes as the device addresses them (host-mapped: kernels read / write the slot in place)
  size_t cap = 0;
  PinnedBuf() {}
  PinnedBuf(PinnedBuf &&o) noexcept { *this = std::move(o); }
  PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(cap, o.cap); return *this; }
  ~PinnedBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    size_t want = bytes + bytes / 4 + 256;
    ZCHK(hipHostMalloc(&p, want, hipHostMallocMapped));
    if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
};

// Process-wide run-time options of the host-pointer entry points (zvec_hip_set_option; environment at first use).
//   wait      how a host-pointer search waits for its stream.  The product calls boundary B from many threads, one query per
//             call (index.cc:605-619): the runtime's spinning hipStreamSynchronize keeps every waiting thread on a CPU, and
//             with more callers than CPUs the threads that have kernels to launch wait for time slices behind them.
//             0 = spin (hipStreamSynchronize), 1 = poll a completion word in pinned memory, yielding the CPU between polls
//             (a one-thread kernel at the end of the chain writes it), 2 = block on an event created with hipEventBlockingSync
//   zerocopy  small transfers skip the copy engine.  bit 1 (value 2, the default): the last kernels write keys | scores | counts
//             into the host-mapped result slot; bit 0: the first kernel reads the query rows from the host-mapped pinned slot —
//             measured SLOWER than the staged copy (single query, 10M x 768: 0.121 against 0.104 ms per call), off by default
struct RuntimeOpts {
  std::atomic<int> wait{1};
  std::atomic<int> zerocopy{2};
  std::atomic<int> assign256{1};     // fp16 labelling on the 256 x 256 multi-phase tile (0: always the 128 x 128 one-barrier tile)
  std::atomic<int> scan256{1};       // wide fp16 flat scans (>= 256 queries, k <= 11) on the 256 x 256 multi-phase tile (0: scan8_kernel; 2: on cache-resident bases too)
  // grouped sparse full scan: a sub-batch of at most this many queries dumps its scores with sparse_rows_dump_kernel (a wave per
  // stored row), a wider one with sparse_scan_kernel (lane = query).  0 = never.  Default: DESIGN §3b "Group-by", from profiles/sparse_grouped*.json
  std::atomic<int> sparse_group_rows{32};
  // how a stale term-major twin of a sparse index is rebuilt: 1 = on the device (zvk_sparse_invb.hip.h), 0 = on the host (the
  // reference of the device build: the same bytes).  Read when a build starts.  DESIGN §3b "Inverted lists"
  std::atomic<int> sparse_inverted_build{1};
  // Hamming IVF search (api_entry_hamming_ivf.inc.h): the partial lists of one slice of a batch stay within this many bytes; a batch
  // that needs more goes in slices of queries.  1 GiB like dense_sub_batch; tests lower it to reach a second slice at small shapes.
  std::atomic<int> bivf_part_bytes{1 << 30};
  // HNSW search (api_entry_hnsw.inc.h): the visited bits and candidate regions of one slice of a batch stay within this many bytes;
  // a batch that needs more goes in slices of queries.  Tests lower it to reach a second slice at small shapes.
  std::atomic<int> hnsw_ws_bytes{1 << 30};
  // HNSW build (api_entry_hnsw_build.inc.h): with s nodes in the graph the next round inserts clamp(s / round_div, 1, round_max) nodes
  // against the graph as it stands; round_div 0 = one node per round (the reference's sequential order).  DESIGN §3c "Building".
  std::atomic<int> hnsw_build_round_div{16};
  std::atomic<int> hnsw_build_round_max{4096};
  RuntimeOpts() {
    if (const char *e = getenv("ZVEC_HIP_SCAN256")) scan256 = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("ZVEC_HIP_WAIT")) wait = std::max(0, std::min(2, atoi(e)));
    if (const char *e = getenv("ZVEC_HIP_ASSIGN256")) assign256 = atoi(e) != 0;
    if (const char *e = getenv("ZVEC_HIP_ZEROCOPY")) zerocopy = std::max(0, std::min(3, atoi(e)));
  }
};
inline RuntimeOpts &ropts() {
  static RuntimeOpts o;
  return o;
}

// reader/writer lock that cannot starve the writer (std::shared_mutex on glibc prefers readers: searches that overlap
// continuously would keep an append waiting): everybody passes a gate, a writer keeps it while the readers drain
class FairSharedMutex {
 public:
  void lock() { gate_.lock(); rw_.lock(); gate_.unlock(); }
  void unlock() { rw_.unlock(); }
  void lock_shared() { gate_.lock(); rw_.lock_shared(); gate_.unlock(); }
  void unlock_shared() { rw_.unlock_shared(); }
 private:
  std::mutex gate_;
  std::shared_mutex rw_;
};

// When the data does not let the half-width pre-selection certify its results (rows within the fp16 rounding of each other, a few
// rows of huge norm under inner product) every search pays the fp16 scan AND the fp32 re-run.  The governor watches the certify
// steps: four in a row that had to re-run more than half of their queries suspend the shadow route for the next 64 searches of the
// index (they read the fp32 rows directly), after which it is tried again.  Results are the same either way; this only bounds the
// cost of data the twin cannot serve.
// It also sizes the pre-selection when the caller left it open (preselect = 0): k' starts at max(32, 3k); six certify steps in a row
// without a single re-run narrow it by 8 (a narrower list is cheaper to keep: flat 1M x 768, batch 256: 194 k QPS at 32, 232 k at 16),
// a step that had to re-run more than 1/32 of its queries widens it by 8 and fixes the width it failed at as the floor from then on.
// Range: max(16, 1.5 k rounded up to 8) .. 64.
struct ShadowGovernor {
  std::atomic<uint32_t> bad{0}, pause{0}, clean{0};
  std::atomic<int> level{0}, floor_level{-8};
  uint32_t kp_auto(uint32_t topk) const {
    const int base = (int)std::max<uint32_t>(32, 3 * topk), lo = (int)std::max<uint32_t>(16, (topk * 3 / 2 + 7) / 8 * 8);
    return (uint32_t)std::min(64, std::max(lo, base + 8 * level.load(std::memory_order_relaxed)));
  }
  void report_width(uint32_t rerun, uint32_t count) {      // one call per certify step of a search whose width was left open
    if (rerun == 0) {
      if (clean.fetch_add(1, std::memory_order_relaxed) + 1 >= 6) {
        clean.store(0, std::memory_order_relaxed);
        const int l = level.load(std::memory_order_relaxed);
        if (l > floor_level.load(std::memory_order_relaxed) && l > -4) level.store(l - 1, std::memory_order_relaxed);
      }
    } else {
      clean.store(0, std::memory_order_relaxed);
      if ((uint64_t)rerun * 32 > count) {
        const int l = level.load(std::memory_order_relaxed);
        floor_level.store(std::max(floor_level.load(std::memory_order_relaxed), l + 1), std::memory_order_relaxed);
        if (l < 4) level.store(l + 1, std::memory_order_relaxed);
      }
    }
  }
  bool allow() {                                     // one call per search that could use the shadow rows
    uint32_t p = pause.load(std::memory_order_relaxed);
    while (p > 0 && !pause.compare_exchange_weak(p, p - 1, std::memory_order_relaxed)) {}
    return p == 0;
  }
  void report(uint32_t rerun, uint32_t count) {      // one call per certify step
    if ((uint64_t)rerun * 2 > count) {
      if (bad.fetch_add(1, std::memory_order_relaxed) + 1 >= 4) { bad.store(0, std::memory_order_relaxed); pause.store(64, std::memory_order_relaxed); }
    } else {
      bad.store(0, std::memory_order_relaxed);
    }
  }
  void reset() {
    bad.store(0, std::memory_order_relaxed); pause.store(0, std::memory_order_relaxed); clean.store(0, std::memory_order_relaxed);
    level.store(0, std::memory_order_relaxed); floor_level.store(-8, std::memory_order_relaxed);
  }
};

// What a scan reads of a blocked, HBM-resident set of rows (flat store, IVF centroids, IVF inverted lists, the fp16 twin): its shape
// and where its arrays are.  Owns nothing and copies freely: the compacted keep-set, the seeding prefix and the twin's rows under the
// store's keys are plain values of it with the fields they override.
inline bool dtype_is_binary(int dtype) { return dtype == ZVEC_HIP_DT_BINARY32 || dtype == ZVEC_HIP_DT_BINARY64; }

struct StoreView {
  uint32_t dim_in = 0;   // element dimension at the ABI (cosine: d+1)
  uint32_t dscan = 0;    // scanned dims
  uint32_t dpad = 0;     // 4-byte WORDS per stored row, multiple of 32 (fp32: dscan up to 32; fp16: dscan up to 64, halved)
  uint32_t elem = 4;     // bytes per element: 4 (fp32) or 2 (fp16)
  bool f16 = false;
  bool bin = false;      // binary rows (Hamming): dim_in counts BITS, dpad = 4 words per 16-byte chunk, [chunk][row] inside a tile (zvk_hamming.hip.h)
  int metric = 0;
  uint64_t n = 0;        // padded positions in use
  float *base = nullptr;
  float *bnorm = nullptr;
  float *extra = nullptr;   // cosine: stored norm column
  uint64_t *keys = nullptr;

  void configure(uint32_t dim, int met, int dtype = ZVEC_HIP_DT_FP32) {
    dim_in = dim;
    metric = met;
    f16 = (dtype == ZVEC_HIP_DT_FP16);
    bin = dtype_is_binary(dtype);
    elem = f16 ? 2 : 4;
    if (bin) {             // a row is dim / 32 words, stored as whole 16-byte chunks: at most 12 bytes of padding per row, no norm column
      dscan = dim;
      dpad = (dim / 32 + 3) / 4 * 4;
      return;
    }
    // cosine rows end with the fp32 norm of the original vector: 1 float, or 2 half slots (cosine_converter.cc:205-212)
    dscan = (met == ZVEC_HIP_METRIC_COSINE) ? dim - (f16 ? 2 : 1) : dim;
    dpad = f16 ? ((dscan + 63) / 64 * 64) / 2 : (dscan + TILE_K - 1) / TILE_K * TILE_K;
  }
  // bytes of a row at the ABI: the one place they are computed
  size_t row_bytes() const { return bin ? (size_t)dim_in / 8 : (size_t)dim_in * elem; }
  uint32_t bin_words() const { return dim_in / 32; }      // binary rows: 32-bit words per row at the ABI ...
  uint32_t bin_chunks() const { return dpad / 4; }        // ... and 16-byte chunks per stored row
};

// The rows an index owns: the view every reader takes (a Store converts to its StoreView), and the four arrays behind the view's
// pointers.  Neither copied nor moved.
struct Store : StoreView {
  uint64_t cap_tiles = 0;
  Store() {}
  Store(const Store &) = delete;

  int reserve(uint64_t rows, hipStream_t stream) {
    uint64_t tiles = (rows + TILE_N - 1) / TILE_N;
    if (tiles <= cap_tiles) return 0;
    uint64_t nt = std::max<uint64_t>(tiles, cap_tiles + cap_tiles / 2 + 1);
    Arrays grown;
    ZRET(grown.base.alloc((size_t)nt * TILE_N * dpad));
    if (!bin) ZRET(grown.bnorm.alloc((size_t)nt * TILE_N));     // (the Hamming scan reads no norms)
    ZRET(grown.keys.alloc((size_t)nt * TILE_N));
    if (metric == ZVEC_HIP_METRIC_COSINE) ZRET(grown.extra.alloc((size_t)nt * TILE_N));
    uint64_t used_tiles = (n + TILE_N - 1) / TILE_N;
    if (used_tiles) {
      ZCHK(hipMemcpyAsync(grown.base, base, (size_t)used_tiles * TILE_N * dpad * sizeof(float), hipMemcpyDeviceToDevice, stream));
      if (grown.bnorm) ZCHK(hipMemcpyAsync(grown.bnorm, bnorm, (size_t)used_tiles * TILE_N * sizeof(float), hipMemcpyDeviceToDevice, stream));
      ZCHK(hipMemcpyAsync(grown.keys, keys, (size_t)used_tiles * TILE_N * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
      if (grown.extra) ZCHK(hipMemcpyAsync(grown.extra, extra, (size_t)used_tiles * TILE_N * sizeof(float), hipMemcpyDeviceToDevice, stream));
      ZCHK(hipStreamSynchronize(stream));
    }
    std::swap(own, grown);               // the old arrays go with `grown` on return: hipFree waits for the device
    point_at_own();
    cap_tiles = nt;
    return 0;
  }
  void release() {
    own = Arrays();
    point_at_own();
    cap_tiles = 0;
  }

 private:
  struct Arrays {
    Scoped<float> base, bnorm, extra;
    Scoped<uint64_t> keys;
  } own;
  void point_at_own() { base = own.base; bnorm = own.bnorm; extra = own.extra; keys = own.keys; }
};

// fp16 twin of an fp32 store at the same positions (own base + bnorm; keys / geometry are the store's): the half-width
// pre-selection of zvec_hip_flat_set_shadow / zvec_hip_ivf_set_shadow (zvk_shadow.hip.h).  Built for the rows present at that
// moment; an index drops it when its rows change.
struct ShadowTwin {
  StoreView st;                        // its rows as a scan reads them (keys and `extra` are never its own: null here)
  bool on = false;
  uint32_t kp = 0;                     // rows pre-selected per query (0: sized by the governor)
  Scoped<ShadowFacts> facts;           // device
  float max_err = 0.f, max_norm = 0.f;
  ShadowGovernor gov;

  void drop() {
    base.release(); bnorm.release(); facts.release();
    st = StoreView();
    on = false;
  }
  // the twin of src's positions [0, n) (whole tiles of them).  Flat store (tile0 == nullptr): its first `rows` positions are rows;
  // IVF lists: every list's first size[l] positions from tile0[l] on.  The other positions become zero rows and feed no fact.
  // Ends with on == true, or holding nothing.
  int build(const StoreView &src, uint64_t n, uint64_t rows, const uint32_t *tile0, const uint32_t *size, uint32_t nlist,
            uint32_t preselect, hipStream_t s) {
    drop();
    StoreView v;
    v.configure(src.dim_in, src.metric, ZVEC_HIP_DT_FP16);
    const uint64_t tiles = (n + TILE_N - 1) / TILE_N, npos = tiles * TILE_N;
    Scoped<float> nb, nn;
    Scoped<ShadowFacts> nf;
    if (nb.alloc((size_t)npos * v.dpad) != 0 || nn.alloc(npos) != 0 || nf.alloc(1) != 0) {
      (void)hipGetLastError();         // (the index goes on searching its own rows)
      return ZVEC_HIP_ERR_NO_MEMORY;
    }
    ZCHK(hipMemsetAsync(nf, 0, sizeof(ShadowFacts), s));
    hipLaunchKernelGGL(shadow_rows_kernel, dim3((unsigned)((npos + 3) / 4)), dim3(256), 0, s, src.base, src.dpad, v.dscan, nb.p,
                       v.dpad, nn.p, npos, tile0, size, nlist, rows, nf.p);
    ZCHK(hipGetLastError());
    ShadowFacts f{};
    ZCHK(hipMemcpyAsync(&f, nf, sizeof(f), hipMemcpyDeviceToHost, s));
    ZCHK(hipStreamSynchronize(s));
    if (!(__builtin_bit_cast(float, f.max_abs) < 65504.f)) return ZVEC_HIP_ERR_UNSUPPORTED;     // rows beyond the half range (or nan)
    max_err = __builtin_bit_cast(float, f.max_err);
    max_norm = __builtin_bit_cast(float, f.max_norm);
    base = std::move(nb); bnorm = std::move(nn); facts = std::move(nf);
    v.n = n; v.base = base; v.bnorm = bnorm;
    st = v;
    kp = preselect;
    gov.reset();
    on = true;
    return 0;
  }
  void info(int *enabled, uint64_t *bytes, float *max_row_error, float *max_row_norm) const {
    if (enabled) *enabled = on ? 1 : 0;
    if (bytes) *bytes = on ? (st.n + TILE_N - 1) / TILE_N * TILE_N * (st.dpad + 1) * sizeof(float) : 0;
    if (max_row_error) *max_row_error = on ? max_err : 0.f;
    if (max_row_norm) *max_row_norm = on ? max_norm : 0.f;
  }
  // k' of a search: the certify step's forced width, else the index's fixed one, else the governor's
  uint32_t pick_kp(uint32_t forced, uint32_t topk) const {
    return std::min<uint32_t>(64, forced ? forced : kp ? kp : gov.kp_auto(topk));     // (shadow_select_kernel: one candidate per lane)
  }
  uint32_t width(uint32_t topk) const { return on ? pick_kp(0, topk) : 0; }

 private:
  Scoped<float> base, bnorm;           // behind st.base / st.bnorm
};

// How a search may use its index's twin: as the index decides, at a forced width (the certify step's second pass over the
// flagged queries), or not at all (the certify step's fp32 re-run; a sliced batch).
struct ShadowMode {
  enum Kind { automatic, forced, fp32_only } kind = automatic;
  uint32_t kp = 0;                     // forced: the width
};

// A context's scratch of the half-width pre-selection: fp16 query rows + norms, per-query rounding facts, the k' pre-selected rows
// of every query (keys | shadow scores | true scores | positions | counts), flags [count] + the flagged count [1]
struct ShadowScratch {
  DevBuf q16, qn16, qinfo, keys, scores, rescored, idx, counts, flags;
  uint32_t count = 0;                  // queries of the last search that went through the twin (0: none)
  uint32_t kp = 0;                     // width that search used
  uint32_t topk = 0;                   // its k
  const ShadowTwin *owner = nullptr;   // the twin it went through: a certify step of another index (or another k) is refused
};

}  // namespace

// Contexts that share a gate take turns on their dominant scan kernel (in call order) while everything else of their
// searches — query preparation, coarse pass, plan, merges, refinement, the caller's exchange — overlaps the other
// context's scan: one event, re-recorded behind every gated scan, waited for in front of the next one.
struct zvec_hip_gate_s {
  int device = 0;
  hipEvent_t ev = nullptr;
  bool armed = false;
  std::mutex mu;
};

// What the last IVF search on a context planned (zvec_hip_ctx_last_ivf_plan): the route it took and, for the tile route, where
// its arrays lie inside ctx->plan (u32 word offsets: the buffer may be reallocated, the offsets hold).  Host bookkeeping only.
struct IvfPlanMark {
  uint32_t route = 0;                      // ZVEC_HIP_IVF_ROUTE_*; 0 = the last search planned nothing that can be read back
  uint32_t scan_threads = 0;               // threads of plan_scan_kernel (tile route)
  uint32_t nq = 0, nlist = 0, nprobe = 0;  // nprobe: probe ranks per query (nlist under brute force)
  uint32_t tpc = 0, rows_per_group = 0, brute_force = 0;
  uint64_t slots_bound = 0;                // what part_s / part_i were sized from
  uint64_t npairs = 0;                     // capacity of csr_q / csr_slot
  size_t words = 0;                        // words of the plan buffer in use
  size_t o_qnprobe = 0, o_qscanned = 0, o_qnslots = 0, o_slotbegin = 0, o_lcount = 0, o_lqoff = 0, o_itemoff = 0, o_ltpc = 0,
         o_total = 0, o_csrq = 0, o_csrslot = 0;
};

struct zvec_hip_ctx_s {
  int device = 0;
  zvec_hip_gate_s *gate = nullptr;
  hipStream_t own = nullptr;
  hipStream_t cur = nullptr;
  std::mutex mu;
  // workspace
  DevBuf gtau, ridx;
  DevBuf seed_keys, seed_scores, seed_counts, seed_idx;   // sample scan that seeds the shared admission bounds
  DevBuf cmp_base, cmp_norm, cmp_extra, cmp_keys, cmp_pos, cmp_cnt;   // compacted keep-set (sparse filters)
  DevBuf qpad, qnorm, part_s, part_i, coarse_keys, coarse_scores, coarse_idx, coarse_cnt;
  DevBuf plan;        // all u32 plan arrays
  DevBuf io_q, io_ex, io_out;                          // staging for host-pointer entry points
  DevBuf io_cq;                                        // ... the coarse-space queries of zvec_hip_ivf_search_coarse
  DevView io_keys, io_scores, io_counts;               // the result arrays inside io_out: ONE copy brings them back
  DevBuf grp_ws, grp_of, grp_out, grp_tab;
  DevBuf direct_pos, direct_keys, direct_scores, direct_idx, direct_cnt;   // small-batch IVF route: positions, stage-1 lists
  ShadowScratch sh;                                    // half-width pre-selection (zvec_hip_*_set_shadow)
  DevBuf sp_plan;                                      // sparse search: query offsets | query-block table (api_entry_sparse.inc.h)
  PinnedBuf sp_pin;                                    // ... its pinned source, and the event behind its last upload
  hipEvent_t sp_ev = nullptr;
  DevBuf sp_ing, sp_ing_pairs;                         // dense rows -> CSR: counts, offsets and status | the pairs (api_entry_sparse_ingest.inc.h)
  // Hamming IVF (api_entry_hamming_ivf.inc.h): probe lists [count][np] | probed lists [count] | rows scanned [count] of the last
  // search, kept for zvec_hip_bivf_last_probes; the plan arrays of its current slice
  DevBuf bivf_probe, bivf_plan;
  const void *bivf_owner = nullptr;                    // the index of that search
  uint32_t bivf_count = 0, bivf_np = 0;
  // ... and stage 1 of the last zvec_hip_bivf_search_fp32 (zvec_hip_bivf_last_candidates): a slice's scratch keys [slice][kc] u64 |
  // positions [count][kc] | Hamming scores [count][kc] | counts [count]
  DevBuf bivf_cand;
  uint32_t bivf_cand_count = 0, bivf_cand_kc = 0, bivf_cand_slice = 0;
  // HNSW search (api_entry_hnsw.inc.h): candidate regions | visited bits of the current slice; {distances computed, nodes expanded}
  // per query of the last search, kept for zvec_hip_hnsw_last_stats
  DevBuf hnsw_ws, hnsw_stats;
  const void *hnsw_owner = nullptr;
  uint32_t hnsw_count = 0, hnsw_slices = 0;
  DevBuf benc;                                         // sign bits of the fp32 queries of zvec_hip_flat_search_fp32[_dev] (api_entry_binary_quant.inc.h)
  DevBuf holes_ex;                                     // caller's exclude set OR the store's holes                      // group-by search: per-group bests / lists, group of every position, results
  PinnedBuf pin_in, pin_out;                           // (transfers up to PIN_LIMIT bytes go through pinned memory)
  const void *io_qp = nullptr;                         // where device code finds the uploaded queries: io_q or the mapped pin_in slot
  bool out_mapped = false;                             // io_keys / io_scores / io_counts point into the mapped pin_out slot
  PinnedBuf done_word;                                 // wait policy 1: completion word (epoch) a one-thread kernel writes
  uint32_t done_epoch = 0;
  uint64_t last_wait_ns = 0;                           // how long the previous call waited: spin (short) or sleep (long) next time
  hipEvent_t block_ev = nullptr;                       // wait policy 2: hipEventBlockingSync
  DevBuf stats;       // per-launch {distinct_rows, pair_rows} u64 x PROFILE_MAX
  uint32_t *q_scanned = nullptr, *q_nprobe = nullptr;  // inside plan
  uint32_t *last_list_count = nullptr;                 // inside plan
  uint32_t last_count = 0;
  IvfPlanMark ivf_plan;                                // the last IVF search's route and plan layout (zvec_hip_ctx_last_ivf_plan)
  // profiling
  bool profile = false;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<double> host_bytes, host_flops;   // flat launches: known on the host
  std::vector<int> launch_is_ivf;
  std::vector<uint32_t> prof_dscan;
  int nprof = 0;
  int cus = 0;
  uint32_t route = 0;                                  // which flat scan route the last user-facing flat search took (ROUTE_*, api_flat_scan.inc.h)
  // (the workspace members free themselves afterwards)
  ~zvec_hip_ctx_s() {
    (void)hipSetDevice(device);
    if (own) (void)hipStreamSynchronize(own);
    if (block_ev) (void)hipEventDestroy(block_ev);
    if (sp_ev) (void)hipEventDestroy(sp_ev);
    for (auto e : ev0) (void)hipEventDestroy(e);
    for (auto e : ev1) (void)hipEventDestroy(e);
    if (own) (void)hipStreamDestroy(own);
  }
};

struct zvec_hip_flat_s {
  int device = 0;
  int dtype = 0;
  Store st;
  // fp16 twin of `st` (zvec_hip_flat_set_shadow): any mutation of the store drops it (the store then searches its own rows until it
  // is set again)
  ShadowTwin shadow;
  zvec_hip_ctx_s *defctx = nullptr;
  std::mutex mu;            // serialises the calls that use defctx's workspace (appends, get_vector)
  // The streamer is searched while it grows (flat_streamer_test.cc TestConcurrentAddAndSearch): searches hold `rw`
  // shared while they read the store's pointers / row count and enqueue their kernels; anything that may move or
  // extend the store holds it exclusive.  A growth reallocation frees the old arrays with hipFree, which waits for
  // the device, so kernels enqueued by earlier searches have finished with them.
  FairSharedMutex rw;
  // Every mutation goes through one FlatWrite (api_entry_ctx_flat.inc.h: the writers' protocol).  finish_synced: the stream is drained, readers need nothing.
  // finish_enqueued (append_dev, append_fp32_dev, adds of up to FAST_ROWS rows): the row count is published while kernels are only
  // enqueued on `append_stream`.  Whoever enqueues on ANOTHER stream next — a reader or a writer — makes that stream wait: it records
  // append_ev behind them if nobody has since the last mutation (append_dirty; readers run concurrently and do so under ev_mu) and
  // waits for the event; the same stream orders itself.  A caller's stream may be gone by then, so its event is recorded by the
  // ending at once.  Writers hold `rw` exclusively, so these fields do not move under a reader.  append_pending is never reset.
  hipEvent_t append_ev = nullptr;
  bool append_pending = false;
  bool append_dirty = false;
  hipStream_t append_stream = nullptr;
  std::mutex ev_mu;
  HoleBits holes;           // add-with-id gaps: FlatStreamerEntity::add_vector_with_id pads [count, id) with kInvalidKey rows (flat_streamer_entity.cc:935-952)
  // single-document adds (the product ingests one add_with_id_impl per document): a ring of pinned slots that the pack
  // kernel reads in place — no staging copy, no allocation, no synchronisation per document
  static constexpr uint32_t FAST_ROWS = 8, RING = 64, RING_GROUP = 16;     // one event per group of slots
  PinnedBuf ring;
  size_t ring_slot_bytes = 0;
  hipEvent_t ring_ev[RING / RING_GROUP] = {};
  bool ring_used[RING / RING_GROUP] = {};
  uint32_t ring_next = 0;
  DevBuf enc;               // zvec_hip_flat_append_fp32[_dev]: the encoded words of a slice of rows, between the encoder and the pack kernel
  // (zvec_hip_flat_destroy has made the device current and idle)
  ~zvec_hip_flat_s() {
    for (uint32_t i = 0; i < RING / RING_GROUP; ++i)
      if (ring_used[i]) (void)hipEventDestroy(ring_ev[i]);
    if (append_ev) (void)hipEventDestroy(append_ev);
    delete defctx;
  }
};

// Sparse rows in CSR form (zvk_sparse.hip.h): what the scan reads, and the four arrays behind it.  A position is a row number;
// keys and exclude bits index positions as in the flat store.  Values are `width` bytes each in HBM (4 = fp32, 2 = fp16: never
// widened).  Neither copied nor moved.
struct SparseStore {
  uint32_t width = 4;         // bytes of a stored value; fixed before the first reserve
  uint64_t n = 0;             // rows
  uint64_t elems = 0;         // stored (index, value) pairs
  uint64_t cap_rows = 0, cap_elems = 0;
  uint64_t *row_off = nullptr;   // [n + 1]
  uint32_t *idx = nullptr;
  void *val = nullptr;        // [elements] of `width` bytes
  uint64_t *keys = nullptr;
  SparseStore() {}
  SparseStore(const SparseStore &) = delete;

  // room for `rows` rows and `elements` pairs; grows geometrically like Store::reserve
  int reserve(uint64_t rows, uint64_t elements, hipStream_t stream) {
    if (rows > cap_rows || row_off == nullptr) {
      const uint64_t nr = std::max<uint64_t>(std::max<uint64_t>(rows, 1), cap_rows + cap_rows / 2 + 1);
      Scoped<uint64_t> off, ks;
      ZRET(off.alloc((size_t)nr + 1));
      ZRET(ks.alloc((size_t)nr));
      if (row_off) {
        ZCHK(hipMemcpyAsync(off, row_off, (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        if (n) ZCHK(hipMemcpyAsync(ks, keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
      } else {
        ZCHK(hipMemsetAsync(off, 0, sizeof(uint64_t), stream));       // row_off[0] = 0
      }
      ZCHK(hipStreamSynchronize(stream));
      std::swap(own.row_off, off);         // the old arrays go with the locals on return: hipFree waits for the device
      std::swap(own.keys, ks);
      row_off = own.row_off; keys = own.keys;
      cap_rows = nr;
    }
    if (elements > cap_elems) {
      const uint64_t ne = std::max<uint64_t>(elements, cap_elems + cap_elems / 2 + 1);
      Scoped<uint32_t> ni;
      Scoped<void> nv;
      ZRET(ni.alloc((size_t)ne));
      ZRET(nv.alloc_bytes((size_t)ne * width));
      if (elems) {
        ZCHK(hipMemcpyAsync(ni, idx, (size_t)elems * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        ZCHK(hipMemcpyAsync(nv, val, (size_t)elems * width, hipMemcpyDeviceToDevice, stream));
        ZCHK(hipStreamSynchronize(stream));
      }
      std::swap(own.idx, ni);
      std::swap(own.val, nv);
      idx = own.idx; val = own.val;
      cap_elems = ne;
    }
    return 0;
  }

  // the capacities reserve(rows, elements) would leave
  void grown(uint64_t rows, uint64_t elements, uint64_t *nr, uint64_t *ne) const {
    *nr = (rows > cap_rows || row_off == nullptr) ? std::max<uint64_t>(std::max<uint64_t>(rows, 1), cap_rows + cap_rows / 2 + 1) : cap_rows;
    *ne = elements > cap_elems ? std::max<uint64_t>(elements, cap_elems + cap_elems / 2 + 1) : cap_elems;
  }
  // Four arrays written whole elsewhere (the splice of zvec_hip_sparse_put: room for nr rows and ne pairs, `rows` rows and
  // `elements` pairs in them) take the place of the store's.  The old ones leave in the arguments and go with them: hipFree waits
  // for the device.
  void adopt(Scoped<uint64_t> &off, Scoped<uint64_t> &ks, Scoped<uint32_t> &ni, Scoped<void> &nv, uint64_t nr, uint64_t ne, uint64_t rows,
             uint64_t elements) {
    std::swap(own.row_off, off); std::swap(own.keys, ks); std::swap(own.idx, ni); std::swap(own.val, nv);
    row_off = own.row_off; keys = own.keys; idx = own.idx; val = own.val;
    cap_rows = nr; cap_elems = ne; n = rows; elems = elements;
  }

 private:
  struct Arrays {
    Scoped<uint64_t> row_off, keys;
    Scoped<uint32_t> idx;
    Scoped<void> val;
  } own;
};

// Term-major twin of a SparseStore (zvec_hip_sparse_set_inverted, zvk_sparse_inv.hip.h): the distinct stored indices, the posting
// offsets, and per posting the storage position and the value as stored.  `want`, `stale` and the arrays change only under the
// handle's exclusive lock; an append marks the twin stale and the next search that needs it rebuilds it (api_entry_sparse_inverted.inc.h).
struct InvertedTwin {
  bool want = false;          // asked for by zvec_hip_sparse_set_inverted
  bool stale = true;          // the arrays do not hold the store's rows
  uint64_t builds = 0;
  uint32_t nterms = 0;
  uint64_t elems = 0;         // postings
  int route = -1;             // the build that made the arrays: 0 host, 1 device; -1 while nothing is built
  uint32_t passes = 0;        // digit passes of that build's sort (0 on the host route)
  double build_ms = 0.0;      // its wall-clock time
  Scoped<uint32_t> terms, ppos;
  Scoped<uint64_t> list_off;
  Scoped<void> pval;
  bool ready() const { return want && !stale; }
  uint64_t bytes() const { return terms.cap + ppos.cap + list_off.cap + pval.cap; }
  void drop() {
    terms.release(); ppos.release(); list_off.release(); pval.release();
    nterms = 0; elems = 0; stale = true;
    route = -1; passes = 0; build_ms = 0.0;
  }
};

struct zvec_hip_sparse_s {
  int device = 0;
  int dtype = 0;            // ZVEC_HIP_DT_FP32 or ZVEC_HIP_DT_FP16: the type of every value pointer of the handle's calls
  int metric = ZVEC_HIP_METRIC_IP;      // ZVEC_HIP_METRIC_IP (InnerProductSparse) or ZVEC_HIP_METRIC_L2 (SquaredEuclideanSparse); fixed at creation
  bool l2() const { return metric == ZVEC_HIP_METRIC_L2; }
  SparseStore st;
  InvertedTwin inv;         // off unless zvec_hip_sparse_set_inverted asked for it
  zvec_hip_ctx_s *defctx = nullptr;
  std::mutex mu;            // serialises the calls that use defctx's workspace (appends, get_vector)
  FairSharedMutex rw;       // searches hold it shared, anything that may move or extend the store exclusive (as zvec_hip_flat_s)
  // add-with-id gaps: FlatSparseStreamerEntity::add_vector_with_id pads [count, id) with empty rows under kInvalidKey (flat_sparse_streamer_entity.cc:708-783)
  HoleBits holes;           // (every mutation of the store goes through one SparseWrite, api_entry_sparse.inc.h)
  // zvec_hip_sparse_put: its device workspace (tables and staged pairs of one call; kept between calls), and what the last
  // successful call did (zvec_hip_sparse_put_info)
  DevBuf put_ws;
  int put_route = -1;
  uint64_t put_moved = 0;
  double put_ms = 0.0;
  // zvec_hip_sparse_append_dev / _append_dense_dev: their device workspace (kept between calls), and what the last successful call
  // did (zvec_hip_sparse_ingest_info)
  DevBuf ing_ws;
  int ing_route = -1;
  uint64_t ing_elems = 0;
  double ing_ms = 0.0;
  ~zvec_hip_sparse_s() { delete defctx; }
};

struct zvec_hip_ivf_s {
  int device = 0;
  int dtype = 0;
  uint32_t dim = 0;
  int metric = 0;
  bool loaded = false;
  bool trained = false;                // centroids present (h_centroids + cent store): labelling possible
  bool filling = false;                // between begin_lists and end_lists of a streamed build
  bool coarse_sep = false;             // the centroid store lives in a space of its own (dimension / metric): zvec_hip_ivf_set_coarse_space
  IvfLayout lay;  // which lists are kept, where they lie in `lists`, the fill's cursors, the deal order (host/ivf_layout.h)
  Store cent;     // centroids as a flat store
  Store lists;    // inverted lists, each padded to whole tiles
  ShadowTwin shadow;                   // fp16 twin of `lists` (zvec_hip_ivf_set_shadow)
  std::vector<char> h_centroids;       // [nlist][dim] in the index element type
  struct Tables {                      // the list tables on the device: built whole by ivf_end_lists, replaced whole
    Scoped<uint32_t> d_size, d_size_global, d_tile0, d_order, d_tail;
    Scoped<uint64_t> d_dense0;
  } tab;
  zvec_hip_ctx_s *defctx = nullptr;
  std::mutex mu;            // serialises the calls that change the index or use defctx's workspace (label_dev, get_vector)
  FairSharedMutex rw;       // searches hold it shared, anything that may move or extend the store exclusive (as zvec_hip_flat_s)
  ~zvec_hip_ivf_s() { delete defctx; }
};
