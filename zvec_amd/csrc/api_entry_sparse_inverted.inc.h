// api_entry_sparse_inverted.inc.h — C ABI entry points and host side of the term-major twin of a sparse index (zvk_sparse_inv.hip.h):
// zvec_hip_sparse_set_inverted / zvec_hip_sparse_inverted_info / _export / _build_info, the two builds (device: zvk_sparse_invb.hip.h;
// host: its reference, the same bytes), and the search route over the twin.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

extern "C++" {
namespace {

// The twin of the rows the store holds now, built on the host: the CSR arrays come down, a stable sort of the elements by index
// (two counting passes over 16 bits each, O(elements); the second is skipped while every index fits 16 bits) leaves every list
// ascending by position, because the elements stand in position order in the CSR arrays; then the four arrays go up.  The caller
// holds h->rw exclusively.  Blocking copies on the null stream: no search of this handle enqueues meanwhile, and the appends that
// wrote the rows have synchronised.  A failure leaves the twin stale (the next search tries again) and the handle otherwise as it was.
// Option "sparse_inverted_build" = 0; the reference the device build is held to, byte for byte.
int sparse_inverted_build_host(zvec_hip_sparse_s *h) {
  const SparseStore &st = h->st;
  InvertedTwin &tw = h->inv;
  if (st.elems > 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (element ordinals are 32-bit in the host sort)
  ZCHK(hipSetDevice(h->device));
  const size_t E = (size_t)st.elems, n = (size_t)st.n;
  std::vector<uint64_t> row_off(n + 1, 0);
  std::vector<uint32_t> idx(E), pos(E), ord(E), tmp;
  std::vector<unsigned char> val(E * st.width);
  if (n) ZCHK(hipMemcpy(row_off.data(), st.row_off, (n + 1) * 8, hipMemcpyDeviceToHost));
  if (E) {
    ZCHK(hipMemcpy(idx.data(), st.idx, E * 4, hipMemcpyDeviceToHost));
    ZCHK(hipMemcpy(val.data(), st.val, E * st.width, hipMemcpyDeviceToHost));
  }
  uint32_t max_idx = 0;
  for (size_t r = 0; r < n; ++r)
    for (uint64_t e = row_off[r]; e < row_off[r + 1]; ++e) pos[(size_t)e] = (uint32_t)r;
  for (size_t e = 0; e < E; ++e) max_idx = std::max(max_idx, idx[e]);
  // stable counting pass by the low 16 bits, then (if any index needs them) by the high 16
  std::vector<size_t> cnt(65537);
  auto pass = [&](const std::vector<uint32_t> *from, std::vector<uint32_t> &to, int shift) {
    std::fill(cnt.begin(), cnt.end(), 0);
    for (size_t i = 0; i < E; ++i) ++cnt[((idx[from ? (*from)[i] : i] >> shift) & 0xffffu) + 1];
    for (size_t b = 0; b < 65536; ++b) cnt[b + 1] += cnt[b];
    for (size_t i = 0; i < E; ++i) {
      const uint32_t e = from ? (*from)[i] : (uint32_t)i;
      to[cnt[(idx[e] >> shift) & 0xffffu]++] = e;
    }
  };
  if (max_idx > 0xffffu) {
    tmp.resize(E);
    pass(nullptr, tmp, 0);
    pass(&tmp, ord, 16);
  } else {
    pass(nullptr, ord, 0);
  }
  // the sorted elements -> terms, list offsets, postings
  std::vector<uint32_t> terms, ppos(E);
  std::vector<uint64_t> list_off;
  std::vector<unsigned char> pval(E * st.width);
  for (size_t i = 0; i < E; ++i) {
    const uint32_t e = ord[i];
    if (i == 0 || idx[e] != terms.back()) {
      terms.push_back(idx[e]);
      list_off.push_back(i);
    }
    ppos[i] = pos[e];
    memcpy(&pval[i * st.width], &val[(size_t)e * st.width], st.width);
  }
  list_off.push_back(E);
  Scoped<uint32_t> d_terms, d_ppos;
  Scoped<uint64_t> d_off;
  Scoped<void> d_val;
  ZRET(upload(d_terms, terms.data(), terms.size()));
  ZRET(upload(d_ppos, ppos.data(), E));
  ZRET(upload(d_off, list_off.data(), list_off.size()));
  ZRET(d_val.alloc_bytes(std::max<size_t>(E * st.width, 1)));
  if (E) ZCHK(hipMemcpy(d_val, pval.data(), E * st.width, hipMemcpyHostToDevice));
  // (the old arrays go with the locals: hipFree waits for the device, so kernels of earlier searches have finished with them)
  tw.terms = std::move(d_terms); tw.ppos = std::move(d_ppos); tw.list_off = std::move(d_off); tw.pval = std::move(d_val);
  tw.nterms = (uint32_t)terms.size();
  tw.elems = E;
  tw.stale = false;
  ++tw.builds;
  return 0;
}

// The exclusive scan of zvk_sparse_invb.hip.h over `n` items of `src`: the sums of the chunks, one work-group over the sums (the sum
// of everything goes to *d_total), the chunks.  `sums` holds a word per chunk.  Enqueues only.
template <typename SRC>
int invb_scan(const SRC &src, uint64_t n, uint32_t *sums, uint32_t *d_total, hipStream_t s) {
  const uint32_t chunks = (uint32_t)((n + INVB_SCAN_CHUNK - 1) / INVB_SCAN_CHUNK);
  hipLaunchKernelGGL((invb_scan_sums_kernel<SRC>), dim3(chunks), dim3(INVB_THREADS), 0, s, src, n, sums);
  hipLaunchKernelGGL(invb_scan_top_kernel, dim3(1), dim3(INVB_THREADS), 0, s, sums, chunks, d_total);
  hipLaunchKernelGGL((invb_scan_chunks_kernel<SRC>), dim3(chunks), dim3(INVB_THREADS), 0, s, src, n, (const uint32_t *)sums);
  ZCHK(hipGetLastError());
  return 0;
}

// The same twin built on the device (option "sparse_inverted_build" = 1, the default): a stable radix sort of (index, element
// ordinal) by 8-bit digits, as many passes as the OR of the indices needs, then positions, heads and postings (zvk_sparse_invb.hip.h).
// Same contract as the host build: the caller holds h->rw exclusively, the call blocks until the twin is complete (null stream),
// a failure (no memory for the scratch included) leaves the twin stale and the handle otherwise as it was, and the four arrays
// have the host build's sizes.  Two words come back to the host: the OR (the pass count decides the launches) and nterms (the
// size of terms[] and list_off[]).  The scratch — two (key, ordinal) buffers of 8 bytes per element, the second only from two
// passes on, the count table and the scan's sums — goes with the locals.  The positions of the elements are expanded into the
// pair buffer that does not hold the sorted pairs (a buffer of their own while there is at most one pass).
int sparse_inverted_build_device(zvec_hip_sparse_s *h, uint32_t *passes_out) {
  const SparseStore &st = h->st;
  InvertedTwin &tw = h->inv;
  if (st.elems > 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (element ordinals and the scan's totals are 32-bit)
  ZCHK(hipSetDevice(h->device));
  const uint64_t E = st.elems;
  hipStream_t s = nullptr;
  Scoped<uint32_t> d_terms, d_ppos;
  Scoped<uint64_t> d_off;
  Scoped<void> d_val;
  uint32_t nterms = 0, passes = 0;
  ZRET(d_ppos.alloc(std::max<size_t>((size_t)E, 1)));
  ZRET(d_val.alloc_bytes(std::max<size_t>((size_t)E * st.width, 1)));
  if (E == 0) {
    ZRET(d_terms.alloc(1));
    ZRET(d_off.alloc(1));
    ZCHK(hipMemset(d_off, 0, sizeof(uint64_t)));
  } else {
    Scoped<uint32_t> words;                                            // [0] OR of the indices, [1] nterms, [2] a scan total nobody reads
    ZRET(words.alloc(4));
    ZCHK(hipMemsetAsync(words, 0, 4 * sizeof(uint32_t), s));
    const uint32_t or_grid = (uint32_t)std::min<uint64_t>((E + INVB_THREADS - 1) / INVB_THREADS, 4096);
    hipLaunchKernelGGL(invb_or_kernel, dim3(or_grid), dim3(INVB_THREADS), 0, s, (const uint32_t *)st.idx, E, (uint32_t *)words);
    ZCHK(hipGetLastError());
    uint32_t or_word = 0;
    ZCHK(hipMemcpy(&or_word, words, sizeof(uint32_t), hipMemcpyDeviceToHost));
    while (passes < 4 && (or_word >> (8 * passes)) != 0) ++passes;     // ceil(bits(OR) / 8)
    const uint32_t nblocks = (uint32_t)((E + INVB_BLOCK - 1) / INVB_BLOCK);
    const uint64_t table_words = (uint64_t)256 * nblocks;
    Scoped<uint32_t> ka, oa, kb, ob, table, sums, pos_own;
    ZRET(sums.alloc((size_t)((std::max<uint64_t>(table_words, E) + INVB_SCAN_CHUNK - 1) / INVB_SCAN_CHUNK)));
    if (passes >= 1) {
      ZRET(ka.alloc((size_t)E));
      ZRET(oa.alloc((size_t)E));
      ZRET(table.alloc((size_t)table_words));
    }
    if (passes >= 2) {
      ZRET(kb.alloc((size_t)E));
      ZRET(ob.alloc((size_t)E));
    }
    const uint32_t *keys = st.idx, *ords = nullptr;                     // (no pass: the elements are sorted as they stand)
    for (uint32_t p = 0; p < passes; ++p) {
      uint32_t *ko = (p & 1) ? kb : ka, *oo = (p & 1) ? ob : oa;
      hipLaunchKernelGGL(invb_hist_kernel, dim3(nblocks), dim3(INVB_THREADS), 0, s, keys, E, 8 * p, (uint32_t *)table, nblocks);
      ZCHK(hipGetLastError());
      ZRET(invb_scan(InvbWords{table.p}, table_words, sums, (uint32_t *)words + 2, s));
      if (p == 0) hipLaunchKernelGGL((invb_scatter_kernel<true>), dim3(nblocks), dim3(INVB_THREADS), 0, s, keys, ords, ko, oo, E, 8 * p,
                                     (const uint32_t *)table, nblocks);
      else hipLaunchKernelGGL((invb_scatter_kernel<false>), dim3(nblocks), dim3(INVB_THREADS), 0, s, keys, ords, ko, oo, E, 8 * p,
                              (const uint32_t *)table, nblocks);
      ZCHK(hipGetLastError());
      keys = ko; ords = oo;
    }
    uint32_t *pos = nullptr;
    if (passes >= 2) pos = ((passes - 1) & 1) ? ka : kb;               // (the pairs' last source: read for the last time by the last scatter)
    else { ZRET(pos_own.alloc((size_t)E)); pos = pos_own; }
    const uint32_t ex_grid = (uint32_t)std::min<uint64_t>((st.n + INVB_THREADS / 64 - 1) / (INVB_THREADS / 64), 16384);
    hipLaunchKernelGGL(invb_expand_kernel, dim3(ex_grid), dim3(INVB_THREADS), 0, s, (const uint64_t *)st.row_off, st.n, E, pos);
    ZCHK(hipGetLastError());
    // heads: their number first (terms[] and list_off[] are sized by it), then the scan again, which scatters them
    const uint32_t hchunks = (uint32_t)((E + INVB_SCAN_CHUNK - 1) / INVB_SCAN_CHUNK);
    InvbHeads heads{keys, nullptr, nullptr};
    hipLaunchKernelGGL((invb_scan_sums_kernel<InvbHeads>), dim3(hchunks), dim3(INVB_THREADS), 0, s, heads, E, (uint32_t *)sums);
    hipLaunchKernelGGL(invb_scan_top_kernel, dim3(1), dim3(INVB_THREADS), 0, s, (uint32_t *)sums, hchunks, (uint32_t *)words + 1);
    ZCHK(hipGetLastError());
    ZCHK(hipMemcpy(&nterms, (uint32_t *)words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (nterms == 0 || nterms > E) return ZVEC_HIP_ERR_RUNTIME;
    ZRET(d_terms.alloc(nterms));
    ZRET(d_off.alloc((size_t)nterms + 1));
    heads.terms = d_terms; heads.list_off = d_off;
    hipLaunchKernelGGL((invb_scan_chunks_kernel<InvbHeads>), dim3(hchunks), dim3(INVB_THREADS), 0, s, heads, E, (const uint32_t *)sums);
    ZCHK(hipGetLastError());
    ZCHK(hipMemcpy(d_off.p + nterms, &E, sizeof(uint64_t), hipMemcpyHostToDevice));
    const uint32_t g_grid = (uint32_t)((E + INVB_THREADS - 1) / INVB_THREADS);
    if (st.width == 2) hipLaunchKernelGGL((invb_gather_kernel<uint16_t>), dim3(g_grid), dim3(INVB_THREADS), 0, s, ords, (const uint32_t *)pos,
                                          static_cast<const uint16_t *>(st.val), E, (uint32_t *)d_ppos, static_cast<uint16_t *>(d_val.p));
    else hipLaunchKernelGGL((invb_gather_kernel<uint32_t>), dim3(g_grid), dim3(INVB_THREADS), 0, s, ords, (const uint32_t *)pos,
                            static_cast<const uint32_t *>(st.val), E, (uint32_t *)d_ppos, static_cast<uint32_t *>(d_val.p));
    ZCHK(hipGetLastError());
    ZCHK(hipStreamSynchronize(s));
  }
  // (the old arrays go with the locals, as in the host build)
  tw.terms = std::move(d_terms); tw.ppos = std::move(d_ppos); tw.list_off = std::move(d_off); tw.pval = std::move(d_val);
  tw.nterms = nterms;
  tw.elems = E;
  tw.stale = false;
  ++tw.builds;
  *passes_out = passes;
  return 0;
}

// one build by the route "sparse_inverted_build" names now; what it was and how long it took is kept for zvec_hip_sparse_inverted_build_info
int sparse_inverted_build(zvec_hip_sparse_s *h) {
  const int route = ropts().sparse_inverted_build.load(std::memory_order_relaxed);
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t passes = 0;
  ZRET(route ? sparse_inverted_build_device(h, &passes) : sparse_inverted_build_host(h));
  h->inv.route = route;
  h->inv.passes = passes;
  h->inv.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// h->rw shared, with the twin current if it is asked for: a stale twin is rebuilt once under the exclusive lock (the flag is read
// again there: another search may have rebuilt it meanwhile), and the flag is read once more under the shared lock, since an append
// may have come in between the two locks.
int sparse_lock_current(zvec_hip_sparse_s *h, std::shared_lock<FairSharedMutex> &r) {
  for (;;) {
    r.lock();
    if (!h->inv.want || !h->inv.stale) return 0;
    r.unlock();
    std::unique_lock<FairSharedMutex> w(h->rw);
    if (h->inv.want && h->inv.stale) ZRET(sparse_inverted_build(h));
  }
}

template <typename VT>
int launch_sparse_inv(const SparseInvArgs &a, uint32_t grid, hipStream_t stream) {
  // (16 KiB of accumulators: no launch attribute needed)
  if (a.exclude) hipLaunchKernelGGL((sparse_inv_kernel<VT, true>), dim3(grid), dim3(64), SPARSE_INV_TILE * sizeof(float), stream, a);
  else hipLaunchKernelGGL((sparse_inv_kernel<VT, false>), dim3(grid), dim3(64), SPARSE_INV_TILE * sizeof(float), stream, a);
  ZCHK(hipGetLastError());
  return 0;
}

// zvec_hip_sparse_search over the twin (sparse_search_locked hands over after its own checks: the merge list fits, st.n > 0, the
// twin is current).  Every score of a sub-batch of queries goes to c->part_s as a [query][stride] matrix, stride = whole tiles;
// merge_kernel selects the lists from it as it does for the row scan's score dump.  +inf marks an excluded position and the
// padding, and never passes the merge: its bound is capped at FLT_MAX.  Enqueues only, except for a wait on the previous plan
// upload of the same context.
int sparse_inverted_search_locked(zvec_hip_sparse_s *h, zvec_hip_ctx_s *c, const uint32_t *q_counts, const uint32_t *d_qidx,
                                  const void *d_qval, uint32_t count, uint32_t topk, float threshold, const uint64_t *d_exclude,
                                  const SearchOut &out, hipStream_t s) {
  const SparseStore &st = h->st;
  const InvertedTwin &tw = h->inv;
  const uint64_t ntiles = (st.n + SPARSE_INV_TILE - 1) / SPARSE_INV_TILE, stride = ntiles * SPARSE_INV_TILE;
  if (stride > 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;       // (a dense row's length is 32-bit in merge_kernel)
  std::vector<uint32_t> q_off((size_t)count + 1, 0u);
  for (uint32_t q = 0; q < count; ++q) q_off[q + 1] = q_off[q] + q_counts[q];
  ZRET(sparse_upload_plan(c, q_off, s));
  const uint32_t sub = dense_sub_batch(count, stride);
  ZRET(c->part_s.ensure((size_t)sub * stride * 4));
  SparseInvArgs a{};
  a.terms = tw.terms; a.list_off = tw.list_off; a.ppos = tw.ppos; a.pval = tw.pval; a.nterms = tw.nterms;
  a.exclude = reinterpret_cast<const uint32_t *>(d_exclude);
  a.q_off = c->sp_plan.as<uint32_t>(); a.q_idx = d_qidx; a.q_val = d_qval;
  a.n = st.n; a.stride = (uint32_t)stride; a.out = c->part_s.as<float>();
  for (uint32_t q0 = 0; q0 < count; q0 += sub) {
    a.q0 = q0; a.nq = std::min(sub, count - q0);
    ZRET(sparse_dispatch(st.width, [&](auto vt) { return launch_sparse_inv<decltype(vt)>(a, (uint32_t)(a.nq * ntiles), s); }));
    ZRET(launch_merge(merge_dense_rows(a.out, a.stride, topk, std::min(threshold, FLT_MAX), st.keys, out_from_row(out, q0, topk)), a.nq, 64, s));
  }
  return 0;
}

}  // namespace
}  // extern "C++"

int zvec_hip_sparse_set_inverted(zvec_hip_sparse_t h, int enable) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (h->l2()) return ZVEC_HIP_ERR_UNSUPPORTED;      // (the distance over the union has no term-at-a-time form without the norm expansion)
  std::lock_guard<std::mutex> g(h->mu);
  std::unique_lock<FairSharedMutex> w(h->rw);
  if (enable) {
    h->inv.want = true;                              // (built by the first search that needs it)
    return 0;
  }
  ZCHK(hipSetDevice(h->device));
  h->inv.want = false;
  h->inv.drop();
  return 0;
}

int zvec_hip_sparse_inverted_info(zvec_hip_sparse_t h, int *enabled, uint64_t *bytes, uint64_t *terms, uint32_t *tile_rows,
                                  uint64_t *builds) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (enabled) *enabled = h->inv.want ? 1 : 0;
  if (bytes) *bytes = h->inv.want ? h->inv.bytes() : 0;
  if (terms) *terms = h->inv.want ? h->inv.nterms : 0;
  if (tile_rows) *tile_rows = SPARSE_INV_TILE;
  if (builds) *builds = h->inv.builds;
  return 0;
}

int zvec_hip_sparse_inverted_export(zvec_hip_sparse_t h, uint32_t *terms, uint64_t terms_cap, uint64_t *list_off, uint32_t *ppos, void *pval,
                                    uint64_t elems_cap, uint64_t *nterms, uint64_t *elems) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  std::shared_lock<FairSharedMutex> r(h->rw, std::defer_lock);
  ZRET(sparse_lock_current(h, r));
  const InvertedTwin &tw = h->inv;
  if (!tw.want) return ZVEC_HIP_ERR_UNSUPPORTED;
  if (nterms) *nterms = tw.nterms;
  if (elems) *elems = tw.elems;
  if (((terms || list_off) && terms_cap < tw.nterms) || ((ppos || pval) && elems_cap < tw.elems)) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  // (blocking copies on the null stream: a build has synchronised, and searches only read the arrays)
  if (terms && tw.nterms) ZCHK(hipMemcpy(terms, tw.terms, (size_t)tw.nterms * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (list_off) ZCHK(hipMemcpy(list_off, tw.list_off, ((size_t)tw.nterms + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (ppos && tw.elems) ZCHK(hipMemcpy(ppos, tw.ppos, (size_t)tw.elems * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (pval && tw.elems) ZCHK(hipMemcpy(pval, tw.pval, (size_t)tw.elems * h->st.width, hipMemcpyDeviceToHost));
  return 0;
}

int zvec_hip_sparse_inverted_build_info(zvec_hip_sparse_t h, int *route, uint32_t *passes, uint32_t *block_elems, double *ms) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (route) *route = h->inv.route;
  if (passes) *passes = h->inv.passes;
  if (block_elems) *block_elems = INVB_BLOCK;
  if (ms) *ms = h->inv.build_ms;
  return 0;
}
