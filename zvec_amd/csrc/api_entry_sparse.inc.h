// api_entry_sparse.inc.h — C ABI entry points: flat index of sparse fp32 / fp16 rows under InnerProductSparse or SquaredEuclideanSparse (zvk_sparse.hip.h)
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

extern "C++" {
namespace {

// A handle's value width (4 = fp32, 2 = fp16) as a type: f(VT()).  With its metric (l2: SquaredEuclideanSparse, else
// InnerProductSparse) as well: f(VT(), std::bool_constant<L2>()).
template <typename F>
int sparse_dispatch(uint32_t width, F &&f) {
  return width == 2 ? f(_Float16()) : f(float());
}
template <typename F>
int sparse_dispatch(uint32_t width, bool l2, F &&f) {
  return sparse_dispatch(width, [&](auto vt) { return l2 ? f(vt, std::true_type()) : f(vt, std::false_type()); });
}

// what every scoring kernel reads (the exclude bitset and the query arrays are device pointers)
SparseOperands sparse_operands(const SparseStore &st, const void *d_exclude, const uint32_t *d_qoff, const uint32_t *d_qidx,
                               const void *d_qval) {
  return {st.row_off, st.idx, st.val, static_cast<const uint32_t *>(d_exclude), d_qoff, d_qidx, d_qval};
}

template <typename VT, bool DUMP, bool L2>
int launch_sparse_scan(const SparseScanArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  ZRET((raise_dynamic_lds<&sparse_scan_kernel<VT, false, DUMP, L2>>(LDS_LIMIT)));
  ZRET((raise_dynamic_lds<&sparse_scan_kernel<VT, true, DUMP, L2>>(LDS_LIMIT)));
  if (a.op.exclude) hipLaunchKernelGGL((sparse_scan_kernel<VT, true, DUMP, L2>), dim3(grid), dim3(64), lds, stream, a);
  else hipLaunchKernelGGL((sparse_scan_kernel<VT, false, DUMP, L2>), dim3(grid), dim3(64), lds, stream, a);
  ZCHK(hipGetLastError());
  return 0;
}

// the same for the handle's value type and metric
template <bool DUMP>
int launch_sparse_scan(const zvec_hip_sparse_s *h, const SparseScanArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  return sparse_dispatch(h->st.width, h->l2(), [&](auto vt, auto l2) {
    return launch_sparse_scan<decltype(vt), DUMP, decltype(l2)::value>(a, grid, lds, stream);
  });
}

template <typename VT, bool L2>
int launch_sparse_rows(const SparseRowsArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  // (indices | values of the longest run, at most 32 KiB: no launch attribute needed)
  if (a.op.exclude) hipLaunchKernelGGL((sparse_rows_kernel<VT, true, L2>), dim3(grid), dim3(64), lds, stream, a);
  else hipLaunchKernelGGL((sparse_rows_kernel<VT, false, L2>), dim3(grid), dim3(64), lds, stream, a);
  ZCHK(hipGetLastError());
  return 0;
}

// Host queries of a host-pointer entry: indices | values in one block, the values `width` bytes each and starting at byte te * 4
// (te = the element count, never 0: an all-empty batch still uploads one unused pair).
void sparse_stage_blob(uint32_t width, uint64_t total, const uint32_t *q_indices, const void *q_values, std::vector<uint32_t> &blob,
                       size_t *te) {
  *te = std::max<size_t>((size_t)total, 1);
  blob.assign(*te + (*te * width + 3) / 4, 0u);
  if (total) {
    memcpy(blob.data(), q_indices, (size_t)total * 4);
    memcpy(blob.data() + *te, q_values, (size_t)total * width);
  }
}

// Runs of a batch as the reference requires them: at most PARAM_FLAT_SPARSE_MAX_DIM_SIZE pairs each, indices STRICTLY ascending
// (the merge join of ComputeInnerProductSparseInSegment, inner_product_matrix.h:2866-2888, advances both sides on a match and
// transform_sparse_format, :2913-2930, counts a segment that goes backwards into the wrong one: unsorted or repeated indices give
// the reference an undefined score, so they are refused here).
int sparse_check_runs(const uint32_t *counts, const uint32_t *indices, uint64_t n, uint64_t *total) {
  uint64_t o = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t c = counts[i];
    if (c > SPARSE_MAX_COUNT) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    if (indices)
      for (uint32_t e = 1; e < c; ++e)
        if (indices[o + e] <= indices[o + e - 1]) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    o += c;
  }
  *total = o;
  return 0;
}

// The queries of a host-pointer entry, after the entry's own pointers and (the plain entries) after count == 0 and topk == 0:
// the batch size, the merge list of merge_k entries (0: none, the grouped entries' lists are group_args_ok's), the runs, and arrays
// where there are pairs.  *total = the queries' pairs.  Allocates and copies nothing.
int sparse_queries_ok(const uint32_t *q_counts, const uint32_t *q_indices, const void *q_values, uint32_t count, uint32_t merge_k,
                      uint64_t *total) {
  if (count > (1u << 19)) return ZVEC_HIP_ERR_OUT_OF_RANGE;          // (query offsets are 32-bit: 2^19 x 4096 elements)
  if (merge_k && !merge_fits(merge_k)) return ZVEC_HIP_ERR_UNSUPPORTED;
  ZRET(sparse_check_runs(q_counts, q_indices, count, total));
  if (*total && (!q_indices || !q_values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return 0;
}

// The listed positions of a by-ids entry (count > 0): the list offsets start at 0 and never descend, and there is an array where
// there are entries.  *maxlen = the longest list, at least 1.
int sparse_lists_ok(const uint32_t *ids, const uint32_t *offsets, uint32_t count, uint32_t *maxlen) {
  if (!offsets || offsets[0] != 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  *maxlen = 1;
  for (uint32_t q = 0; q < count; ++q) {
    if (offsets[q + 1] < offsets[q]) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    *maxlen = std::max(*maxlen, offsets[q + 1] - offsets[q]);
  }
  if (offsets[count] && !ids) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return 0;
}

// Query blocks, greedily: consecutive queries while there are at most SPARSE_QB of them and their runs fit the LDS image; a block
// never crosses a multiple of `sub` (the dump route's sub-batches; 0 = none).  plan = q_off[count + 1] | blk[blocks + 1].
void sparse_make_plan(const uint32_t *counts, uint32_t count, uint32_t sub, std::vector<uint32_t> &plan, uint32_t *nblocks, uint32_t *max_img) {
  plan.assign((size_t)count + 1, 0u);
  for (uint32_t q = 0; q < count; ++q) plan[q + 1] = plan[q] + counts[q];
  std::vector<uint32_t> blk(1, 0u);
  uint32_t in_blk = 0, elems = 0, mx = 0;
  for (uint32_t q = 0; q < count; ++q) {
    if (in_blk && (in_blk == SPARSE_QB || elems + counts[q] > SPARSE_IMG_ELEMS || (sub && q % sub == 0))) {
      blk.push_back(q);
      in_blk = 0;
      elems = 0;
    }
    ++in_blk;
    elems += counts[q];
    mx = std::max(mx, elems);
  }
  blk.push_back(count);
  *nblocks = (uint32_t)blk.size() - 1;
  *max_img = mx;
  plan.insert(plan.end(), blk.begin(), blk.end());
}

// The host-made plan of a search goes to c->sp_plan through the context's pinned slot: the previous search's upload has to have
// left it (the only wait of the search paths below).
int sparse_upload_plan(zvec_hip_ctx_s *c, const std::vector<uint32_t> &plan, hipStream_t s) {
  if (c->sp_ev == nullptr) ZCHK(hipEventCreateWithFlags(&c->sp_ev, hipEventDisableTiming));
  else ZCHK(hipEventSynchronize(c->sp_ev));
  ZRET(c->sp_pin.ensure(plan.size() * 4));
  ZRET(c->sp_plan.ensure(plan.size() * 4));
  memcpy(c->sp_pin.p, plan.data(), plan.size() * 4);
  ZCHK(hipMemcpyAsync(c->sp_plan.p, c->sp_pin.p, plan.size() * 4, hipMemcpyHostToDevice, s));
  ZCHK(hipEventRecord(c->sp_ev, s));
  return 0;
}

// sparse_scan_kernel's grid: one wave per work-group, 8 of them per CU, a chunk of rows per work-group and query block.
// part_k != 0 (the fused route): the partial lists of `count` queries, part_k entries each, take at most 64 MiB (a wide batch with
// long lists gets longer chunks).
void sparse_chunking(zvec_hip_ctx_s *c, uint64_t n, uint32_t nqb, uint32_t count, uint32_t part_k, uint32_t *rpc, uint32_t *nchunks) {
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)device_cus(c) * 8 + nqb - 1) / nqb);
  uint64_t r = std::max<uint64_t>(1, (n + want - 1) / want);
  while (part_k && (uint64_t)count * ((n + r - 1) / r) * part_k * 8 > (64ull << 20) && r < n) r *= 2;
  *rpc = (uint32_t)std::min<uint64_t>(r, 0x7fffffffu);
  *nchunks = (uint32_t)((n + *rpc - 1) / *rpc);
}

// Every score of the queries [q0, q0 + cnt) of a planned batch: dump[(q - q0) * n + position], +inf for an excluded position,
// through sparse_scan_kernel<.., DUMP> (lane = query; it reads no k, threshold or shared bound).  plan = sparse_make_plan's for
// `count` queries, uploaded behind op.q_off; its blocks cross neither q0 nor q0 + cnt (the plan's `sub`), so the sub-batch is the
// blocks [b0, b1).
int sparse_dump_scores(const zvec_hip_sparse_s *h, zvec_hip_ctx_s *c, const SparseOperands &op, const std::vector<uint32_t> &plan,
                       uint32_t count, uint32_t max_img, uint32_t q0, uint32_t cnt, float *dump, hipStream_t s) {
  const auto blk = plan.begin() + count + 1;
  const uint32_t b0 = (uint32_t)(std::lower_bound(blk, plan.end(), q0) - blk);
  const uint32_t b1 = (uint32_t)(std::lower_bound(blk, plan.end(), q0 + cnt) - blk);
  SparseScanArgs a{};
  a.op = op; a.blk = op.q_off + count + 1; a.blk0 = b0; a.qsub0 = q0; a.nqblocks = b1 - b0; a.n = h->st.n; a.dump = dump;
  sparse_chunking(c, a.n, a.nqblocks, count, 0, &a.rows_per_chunk, &a.nchunks);
  return launch_sparse_scan<true>(h, a, a.nchunks * a.nqblocks, sparse_lds_bytes(max_img, 0, h->st.width), s);
}

// api_entry_sparse_inverted.inc.h: the term-major twin.  sparse_lock_current takes h->rw shared with the twin current if it is
// asked for (it rebuilds a stale one under the exclusive lock first); sparse_inverted_search_locked is the search over it.
int sparse_lock_current(zvec_hip_sparse_s *h, std::shared_lock<FairSharedMutex> &r);
int sparse_inverted_search_locked(zvec_hip_sparse_s *h, zvec_hip_ctx_s *c, const uint32_t *q_counts, const uint32_t *d_qidx,
                                  const void *d_qval, uint32_t count, uint32_t topk, float threshold, const uint64_t *d_exclude,
                                  const SearchOut &out, hipStream_t s);

// The search proper.  The caller holds c->mu and h->rw (shared, through sparse_lock_current); q_counts (HOST) has passed
// sparse_check_runs; the query arrays and every output are device pointers.  Enqueues only, except for a wait on the previous plan
// upload of the same context.
int sparse_search_locked(zvec_hip_sparse_s *h, zvec_hip_ctx_s *c, const uint32_t *q_counts, const uint32_t *d_qidx, const void *d_qval,
                         uint32_t count, uint32_t topk, float threshold, const uint64_t *d_exclude, uint64_t *d_keys, float *d_scores,
                         uint32_t *d_counts, hipStream_t s) {
  if (!merge_fits(topk)) return ZVEC_HIP_ERR_UNSUPPORTED;
  const SparseStore &st = h->st;
  if (st.n == 0) return empty_results(d_keys, d_counts, count, topk, s);
  ZRET(effective_exclude(h->holes, st.n, c, d_exclude, s, &d_exclude));      // (the caller's pointer untouched while the store has no hole)
  const SearchOut out{d_keys, d_scores, nullptr, d_counts};
  if (h->inv.ready()) return sparse_inverted_search_locked(h, c, q_counts, d_qidx, d_qval, count, topk, threshold, d_exclude, out, s);
  const bool dump = topk > SPARSE_FUSED_MAX_K;
  const uint32_t sub = dump ? dense_sub_batch(count, st.n) : 0u;      // (a dumped row is the st.n scores of one query)
  std::vector<uint32_t> plan;
  uint32_t nblocks = 0, max_img = 0;
  sparse_make_plan(q_counts, count, sub, plan, &nblocks, &max_img);
  ZRET(sparse_upload_plan(c, plan, s));
  ZRET(c->gtau.ensure((size_t)count * 4));
  hipLaunchKernelGGL(sparse_prep_queries_kernel, dim3((count + 255) / 256), dim3(256), 0, s, count, c->gtau.as<uint32_t>());
  ZCHK(hipGetLastError());

  const SparseOperands op = sparse_operands(st, d_exclude, c->sp_plan.as<uint32_t>(), d_qidx, d_qval);
  if (dump) {
    ZRET(c->part_s.ensure((size_t)sub * st.n * 4));
    for (uint32_t q0 = 0; q0 < count; q0 += sub) {
      const uint32_t cnt = std::min(sub, count - q0);
      ZRET(sparse_dump_scores(h, c, op, plan, count, max_img, q0, cnt, c->part_s.as<float>(), s));
      ZRET(launch_merge(merge_dense_rows(c->part_s.as<float>(), (uint32_t)st.n, topk, threshold, st.keys, out_from_row(out, q0, topk)), cnt, 64, s));
    }
    return 0;
  }
  SparseScanArgs a{};
  a.op = op; a.blk = op.q_off + count + 1; a.k = topk; a.threshold = threshold; a.n = st.n; a.gtau = c->gtau.as<uint32_t>();
  a.nqblocks = nblocks;
  sparse_chunking(c, st.n, nblocks, count, topk, &a.rows_per_chunk, &a.nchunks);
  const uint64_t slots = (uint64_t)count * a.nchunks;
  ZRET(c->part_s.ensure(slots * topk * sizeof(float)));
  ZRET(c->part_i.ensure(slots * topk * sizeof(uint32_t)));
  a.part_s = c->part_s.as<float>(); a.part_i = c->part_i.as<uint32_t>();
  ZRET(launch_sparse_scan<false>(h, a, a.nchunks * nblocks, sparse_lds_bytes(max_img, topk, st.width), s));
  return launch_merge(merge_partials(a.part_s, a.part_i, a.nchunks, a.gtau, topk, threshold, st.keys, out), count, merge_threads(count), s);
}

// Scores of listed rows (sparse_rows_kernel): query q against the positions ids[offsets[q] .. offsets[q + 1]).  The caller holds
// c->mu and h->rw (shared); q_counts, ids and offsets are HOST arrays, q_counts has passed sparse_check_runs and offsets starts at 0
// and never descends; the query arrays and the bitset are device pointers.  Leaves the scores in c->part_s [entries] (+inf: position
// beyond the rows, excluded, or a hole), the positions in c->plan [entries] and tells where the list offsets went (*d_list_off).  Enqueues
// only, except for a wait on the previous plan upload of the same context.  A work item is (query, slice of its list): the slice is
// as long as it takes to put 16 items on every CU, SPARSE_ROWS_SLICE at most, so that a short batch still fills the device.
// row_stride != 0 (the grouped search; >= the longest list): the scores go to c->part_s as a [count][row_stride] matrix instead,
// entry j of query q's list at q * row_stride + j, and the scored positions to c->part_i in the same layout; padding and skipped
// entries hold +inf and IDX_NONE.
int sparse_rows_locked(zvec_hip_sparse_s *h, zvec_hip_ctx_s *c, const uint32_t *q_counts, const uint32_t *d_qidx, const void *d_qval,
                       uint32_t count, const uint32_t *ids, const uint32_t *offsets, const uint64_t *d_exclude,
                       const uint32_t **d_list_off, hipStream_t s, uint32_t row_stride = 0) {
  const SparseStore &st = h->st;
  ZRET(effective_exclude(h->holes, st.n, c, d_exclude, s, &d_exclude));      // (a hole is never scored: +inf, as any excluded position)
  const uint32_t total = offsets[count];
  const uint64_t want = (uint64_t)device_cus(c) * 16;
  const uint32_t slice = (uint32_t)std::min<uint64_t>(SPARSE_ROWS_SLICE, std::max<uint64_t>(1, (total + want - 1) / want));
  // plan = q_off[count + 1] | list_off[count + 1] | item_q[items] | item_e0[items]
  std::vector<uint32_t> plan((size_t)2 * (count + 1), 0u), item_e0;
  uint32_t max_run = 0;
  for (uint32_t q = 0; q < count; ++q) {
    plan[q + 1] = plan[q] + q_counts[q];
    max_run = std::max(max_run, q_counts[q]);
  }
  memcpy(plan.data() + count + 1, offsets, ((size_t)count + 1) * 4);
  for (uint32_t q = 0; q < count; ++q)
    for (uint64_t e = offsets[q]; e < offsets[q + 1]; e += slice) {
      plan.push_back(q);
      item_e0.push_back((uint32_t)e);
    }
  const uint32_t items = (uint32_t)item_e0.size();
  plan.insert(plan.end(), item_e0.begin(), item_e0.end());
  ZRET(sparse_upload_plan(c, plan, s));
  c->ivf_plan.route = 0;        // (the plan buffer is reused: no IVF plan to read back any more)
  ZRET(c->plan.ensure(std::max<size_t>(total, 1) * 4));
  const size_t cells = row_stride ? (size_t)count * row_stride : std::max<size_t>(total, 1);
  ZRET(c->part_s.ensure(cells * 4));
  if (row_stride) {
    ZRET(c->part_i.ensure(cells * 4));
    ZCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->part_s.p), 0x7f800000, cells, s));      // +inf
    ZCHK(hipMemsetAsync(c->part_i.p, 0xff, cells * 4, s));                                             // IDX_NONE
  }
  if (total) ZCHK(hipMemcpyAsync(c->plan.p, ids, (size_t)total * 4, hipMemcpyHostToDevice, s));
  SparseRowsArgs a{};
  a.op = sparse_operands(st, d_exclude, c->sp_plan.as<uint32_t>(), d_qidx, d_qval);
  a.ids = c->plan.as<uint32_t>(); a.list_off = a.op.q_off + count + 1; a.item_q = a.list_off + count + 1; a.item_e0 = a.item_q + items;
  a.slice = slice; a.n = st.n; a.scores = c->part_s.as<float>(); a.row_stride = row_stride; a.pos_out = c->part_i.as<uint32_t>();
  *d_list_off = a.list_off;
  if (items == 0) return 0;
  return sparse_dispatch(st.width, h->l2(), [&](auto vt, auto l2) {
    return launch_sparse_rows<decltype(vt), decltype(l2)::value>(a, items, sparse_run_lds_bytes(max_run, st.width), s);
  });
}

// One mutation of a sparse store: FlatWrite's twin on the handle's own stream, which every entry drains itself.  It holds h->mu, then
// h->rw exclusively, while it lives; cover() as HoleBits says; finish() ends an entry that changed the store (the next search rebuilds the twin).
struct SparseWrite {
  zvec_hip_sparse_s *const h;
  hipStream_t const s;
  explicit SparseWrite(zvec_hip_sparse_s *h_) : h(h_), s(h_->defctx->own), g(h_->mu), w(h_->rw) {}
  int open() { ZCHK(hipSetDevice(h->device)); return 0; }
  int cover(uint64_t rows, bool leaves = false) { return h->holes.reserve(rows, leaves, s); }
  int finish() { h->inv.stale = true; return h->holes.upload_dirty(s); }
 private:
  std::lock_guard<std::mutex> g;
  std::unique_lock<FairSharedMutex> w;
};

}  // namespace
}  // extern "C++"

int zvec_hip_sparse_create_metric(int dtype, int metric, int device, zvec_hip_sparse_t *out) {
  if (!out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (dtype != ZVEC_HIP_DT_FP32 && dtype != ZVEC_HIP_DT_FP16) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (metric != ZVEC_HIP_METRIC_IP && metric != ZVEC_HIP_METRIC_L2) return ZVEC_HIP_ERR_UNSUPPORTED;
  zvec_hip_ctx_s *c = nullptr;
  ZRET(ctx_new(device, &c));
  zvec_hip_sparse_s *h = new (std::nothrow) zvec_hip_sparse_s();
  if (!h) { ctx_free(c); return ZVEC_HIP_ERR_NO_MEMORY; }
  h->device = device; h->dtype = dtype; h->metric = metric; h->defctx = c;
  h->st.width = dtype == ZVEC_HIP_DT_FP16 ? 2u : 4u;
  *out = h;
  return 0;
}

int zvec_hip_sparse_create_typed(int dtype, int device, zvec_hip_sparse_t *out) {
  return zvec_hip_sparse_create_metric(dtype, ZVEC_HIP_METRIC_IP, device, out);
}

int zvec_hip_sparse_create(int device, zvec_hip_sparse_t *out) {
  return zvec_hip_sparse_create_metric(ZVEC_HIP_DT_FP32, ZVEC_HIP_METRIC_IP, device, out);
}

int zvec_hip_sparse_metric(zvec_hip_sparse_t h, int *metric) {
  if (!h || !metric) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  *metric = h->metric;
  return 0;
}

int zvec_hip_sparse_dtype(zvec_hip_sparse_t h, int *dtype) {
  if (!h || !dtype) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  *dtype = h->dtype;
  return 0;
}

int zvec_hip_sparse_destroy(zvec_hip_sparse_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  delete h;
  return 0;
}

int zvec_hip_sparse_reserve(zvec_hip_sparse_t h, uint64_t rows, uint64_t elements) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  SparseWrite w(h);
  ZRET(w.open());
  return h->st.reserve(rows, elements, w.s);             // (no row is stored: nothing to cover, and the twin still holds the rows)
}

int zvec_hip_sparse_append(zvec_hip_sparse_t h, const uint32_t *counts, const uint32_t *indices, const void *values, uint64_t n,
                           const uint64_t *keys) {
  if (!h || (n && !counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  uint64_t total = 0;
  ZRET(sparse_check_runs(counts, indices, n, &total));       // (before anything is stored: a refused call stores nothing)
  if (total && (!indices || !values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  SparseWrite w(h);
  SparseStore &st = h->st;
  if (st.n + n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (positions are 32-bit in the partial lists)
  ZRET(w.open());
  hipStream_t s = w.s;
  ZRET(w.cover(st.n + n));
  ZRET(st.reserve(st.n + n, st.elems + total, s));
  // one copy per array: offsets (the first one is the old end, already there), keys, indices, values
  std::vector<uint64_t> off((size_t)n), ks;
  uint64_t o = st.elems;
  for (uint64_t i = 0; i < n; ++i) off[i] = (o += counts[i]);
  if (!keys) {
    ks.resize((size_t)n);
    for (uint64_t i = 0; i < n; ++i) ks[i] = st.n + i;
  }
  ZCHK(hipMemcpyAsync(st.row_off + st.n + 1, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  ZCHK(hipMemcpyAsync(st.keys + st.n, keys ? keys : ks.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  if (total) {
    ZCHK(hipMemcpyAsync(st.idx + st.elems, indices, (size_t)total * 4, hipMemcpyHostToDevice, s));
    ZCHK(hipMemcpyAsync(static_cast<char *>(st.val) + st.elems * st.width, values, (size_t)total * st.width, hipMemcpyHostToDevice, s));
  }
  ZCHK(hipStreamSynchronize(s));
  st.n += n;
  st.elems += total;
  return w.finish();
}

int zvec_hip_sparse_count(zvec_hip_sparse_t h, uint64_t *rows, uint64_t *elements) {
  if (!h || (!rows && !elements)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (rows) *rows = h->st.n;
  if (elements) *elements = h->st.elems;
  return 0;
}

int zvec_hip_sparse_get_vector(zvec_hip_sparse_t h, uint64_t pos, uint32_t *count, uint32_t *indices, void *values) {
  if (!h || !count) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(h->mu);
  zvec_hip_ctx_s *c = h->defctx;
  std::lock_guard<std::mutex> gc(c->mu);             // io_q is the built-in context's staging buffer
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (pos >= h->st.n) return ZVEC_HIP_ERR_NO_EXIST;
  ZCHK(hipSetDevice(h->device));
  const size_t words = 4 + 2 * (size_t)SPARSE_MAX_COUNT;
  ZRET(c->io_q.ensure(words * 4));
  ZRET(sparse_dispatch(h->st.width, [&](auto vt) -> int {
    using VT = decltype(vt);
    hipLaunchKernelGGL(sparse_unpack_kernel<VT>, dim3(1), dim3(256), 0, c->own, h->st.row_off, h->st.idx, static_cast<const VT *>(h->st.val),
                       pos, c->io_q.as<uint32_t>());
    ZCHK(hipGetLastError());
    return 0;
  }));
  std::vector<uint32_t> host(words);
  ZCHK(hipMemcpyAsync(host.data(), c->io_q.p, words * 4, hipMemcpyDeviceToHost, c->own));
  ZCHK(hipStreamSynchronize(c->own));
  *count = host[0];
  if (indices) memcpy(indices, host.data() + 4, (size_t)host[0] * 4);
  if (values) memcpy(values, host.data() + 4 + SPARSE_MAX_COUNT, (size_t)host[0] * h->st.width);
  return 0;
}

int zvec_hip_sparse_search_dev(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *d_q_indices,
                               const void *d_q_values, uint32_t count, uint32_t topk, float threshold, const uint64_t *d_exclude_bitset,
                               uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream) {
  if (!h || !d_out_keys || !d_out_scores || !d_out_counts || (count && !q_counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count > (1u << 19)) return ZVEC_HIP_ERR_OUT_OF_RANGE;          // (query offsets are 32-bit: 2^19 x 4096 elements)
  uint64_t total = 0;
  ZRET(sparse_check_runs(q_counts, nullptr, count, &total));
  if (total && (!d_q_indices || !d_q_values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  ZCHK(hipSetDevice(h->device));
  std::shared_lock<FairSharedMutex> r(h->rw, std::defer_lock);
  ZRET(sparse_lock_current(h, r));
  return sparse_search_locked(h, c, q_counts, d_q_indices, d_q_values, count, topk, threshold, d_exclude_bitset, d_out_keys, d_out_scores,
                              d_out_counts, pick_stream(c, stream));
}

int zvec_hip_sparse_search(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                           const void *q_values, uint32_t count, uint32_t topk, float threshold, const uint64_t *exclude_bitset,
                           uint64_t *out_keys, float *out_scores, uint32_t *out_counts) {
  if (!h || !out_keys || !out_scores || !out_counts || (count && !q_counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  uint64_t total = 0;
  ZRET(sparse_queries_ok(q_counts, q_indices, q_values, count, topk, &total));
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->st.width, total, q_indices, q_values, blob, &te);      // (the width never changes after create)
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw, std::defer_lock);      // the row count the bitset is sized for == the rows scanned
    ZRET(sparse_lock_current(h, r));
    ZRET(host_search_wrap_begin(c, blob.data(), blob.size() * 4, exclude_bitset, h->st.n, count, topk, c->cur));
    const uint32_t *dq = static_cast<const uint32_t *>(c->io_qp);
    ZRET(sparse_search_locked(h, c, q_counts, dq, dq + te, count, topk, threshold,
                              exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr, c->io_keys.as<uint64_t>(), c->io_scores.as<float>(),
                              c->io_counts.as<uint32_t>(), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

// FlatSparseStreamer::search_bf_by_p_keys_impl (flat_sparse_streamer.cc:324-349; FlatSparseSearcher's, flat_sparse_searcher.cc:
// 98-103; FlatSparseEntity::search_p_keys, flat_sparse_entity.h:63-77): query q is scored against the rows at positions
// ids[offsets[q] .. offsets[q + 1]) only.  The caller has mapped primary keys to positions and dropped unknown keys (get_id(p_key)
// == kInvalidNodeId); a position beyond the rows is skipped here, a position listed twice is scored twice (the reference's heap
// takes both emplace calls).
int zvec_hip_sparse_search_by_ids(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                                  const void *q_values, uint32_t count, const uint32_t *ids, const uint32_t *offsets, uint32_t topk,
                                  float threshold, const uint64_t *exclude_bitset, uint64_t *out_keys, float *out_scores,
                                  uint32_t *out_counts) {
  if (!h || !out_keys || !out_scores || !out_counts || (count && (!q_counts || !offsets))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  uint64_t total = 0;
  uint32_t maxlen = 0;
  ZRET(sparse_queries_ok(q_counts, q_indices, q_values, count, topk, &total));
  ZRET(sparse_lists_ok(ids, offsets, count, &maxlen));       // (the longest list is of no use here)
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->st.width, total, q_indices, q_values, blob, &te);      // (the width never changes after create)
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  ZCHK(hipSetDevice(h->device));
  {
    std::shared_lock<FairSharedMutex> r(h->rw);      // the row count the bitset is sized for == the rows the positions are checked against
    ZRET(host_search_wrap_begin(c, blob.data(), blob.size() * 4, exclude_bitset, h->st.n, count, topk, c->cur));
    const uint32_t *dq = static_cast<const uint32_t *>(c->io_qp);
    const uint32_t *d_off = nullptr;
    ZRET(sparse_rows_locked(h, c, q_counts, dq, dq + te, count, ids, offsets,
                            exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr, &d_off, c->cur));
    // selection, the threshold test and position -> key: every listed entry is a slot of one candidate, a query's slots are its list
    // (a skipped entry holds +inf, which no finite bound admits)
    const SearchOut out{c->io_keys.as<uint64_t>(), c->io_scores.as<float>(), nullptr, c->io_counts.as<uint32_t>()};
    ZRET(launch_merge(merge_slot_ranges(c->part_s.as<float>(), c->plan.as<uint32_t>(), d_off, 1, nullptr, topk, std::min(threshold, FLT_MAX),
                                        h->st.keys, out), count, merge_threads(count), c->cur));
  }
  return host_search_wrap_end(c, count, topk, out_keys, out_scores, out_counts, c->cur);
}

// IndexMetric::batch_distance (index_metric.h:85-87) for sparse rows: ONE query against n listed positions, scores only, in the
// listed order (sparse_rows_kernel without the selection; FlatSparseEntity::search_p_keys, flat_sparse_entity.h:63-77, scores its
// keys one by one the same way).  A position beyond the rows scores +inf.
int zvec_hip_sparse_batch_distance(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, uint32_t q_count, const uint32_t *q_indices,
                                   const void *q_values, const uint32_t *positions, uint32_t n, float *out_scores) {
  if (!h || (q_count && (!q_indices || !q_values)) || (n && (!positions || !out_scores))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  uint64_t total = 0;
  ZRET(sparse_check_runs(&q_count, q_indices, 1, &total));
  if (n == 0) return 0;
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->st.width, total, q_indices, q_values, blob, &te);
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = c->cur;
  ZRET(c->io_q.ensure(blob.size() * 4));
  ZCHK(hipMemcpyAsync(c->io_q.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, s));
  const uint32_t *dq = c->io_q.as<uint32_t>();
  const uint32_t offs[2] = {0, n};
  const uint32_t *d_off = nullptr;
  ZRET(sparse_rows_locked(h, c, &q_count, dq, dq + te, 1, positions, offs, nullptr, &d_off, s));
  ZCHK(hipMemcpyAsync(out_scores, c->part_s.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipStreamSynchronize(s));
  return 0;
}
