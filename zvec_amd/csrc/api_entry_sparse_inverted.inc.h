// api_entry_sparse_inverted.inc.h — C ABI entry points and host side of the term-major twin of a sparse index (zvk_sparse_inv.hip.h):
// zvec_hip_sparse_set_inverted / zvec_hip_sparse_inverted_info, the host build, and the search route over the twin.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

extern "C++" {
namespace {

// The twin of the rows the store holds now, built on the host: the CSR arrays come down, a stable sort of the elements by index
// (two counting passes over 16 bits each, O(elements); the second is skipped while every index fits 16 bits) leaves every list
// ascending by position, because the elements stand in position order in the CSR arrays; then the four arrays go up.  The caller
// holds h->rw exclusively.  Blocking copies on the null stream: no search of this handle enqueues meanwhile, and the appends that
// wrote the rows have synchronised.  A failure leaves the twin stale (the next search tries again) and the handle otherwise as it was.
int sparse_inverted_build(zvec_hip_sparse_s *h) {
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
