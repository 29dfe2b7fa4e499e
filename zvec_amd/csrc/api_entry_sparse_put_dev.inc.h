// api_entry_sparse_put_dev.inc.h — C ABI entry point: add-with-id on a sparse index with the call's rows in device memory
// (zvec_hip_sparse_put_dev; device side: zvk_sparse_put.hip.h, the checks of zvk_sparse_ingest.hip.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// zvec_hip_sparse_put (api_entry_sparse_put.inc.h) with the host's share of the pairs taken away.  What that entry does on the host
// with the pairs — the run check and the stage — is done on the device here, by the scan and check of zvec_hip_sparse_append_dev and
// by sparse_put_stage_kernel; what it does with one word a row stays on the host: the sort by id, the keep-last rule, the route, the
// hole bits and the sizes of the allocations.  So
//   scan of d_counts -> sparse_csr_check_kernel -> sparse_put_lens_kernel (the old lengths at the call's ids)
//   ONE wait: the status word, the total, and per row its id, its count and its old length (12 bytes a row)
//   the plan goes up (tid, src, tval, sb: 24 bytes a kept row) -> sparse_put_stage_kernel (stage and keys) -> for overwritten rows
//   sparse_put_pieces_kernel (tbeg, ds, ss from the store's own offsets) -> the route's kernels exactly as the host put launches
//   them -> drained, then counts, hole bits and put_info.
// Neither d_indices, d_values nor d_keys is read by the host.  The stage, the tables and so the store are the host put's, bit for bit.

extern "C++" {
namespace {

int sparse_put_dev(zvec_hip_sparse_s *h, const uint32_t *d_ids, const uint32_t *d_counts, const uint32_t *d_indices, const void *d_values,
                   uint64_t n, uint64_t elements, const uint64_t *d_keys, void *stream) {
  if (!h || (n && (!d_ids || !d_counts))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  if (elements && (!d_indices || !d_values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  SparseWrite w(h);
  SparseStore &st = h->st;
  const uint32_t width = st.width;
  ZRET(w.open());
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w.s;
  const uint64_t old_n = st.n, old_elems = st.elems;

  // the checks, and the three words a row the plan is made from
  IngestWs iw;
  ZRET(ingest_ws(h->ing_ws, n, false, 0, &iw));
  ZRET(h->put_ws.ensure((size_t)n * 4));
  std::vector<uint32_t> hw((size_t)n * 3);                             // ids | counts | old lengths
  const uint32_t *ids = hw.data(), *counts = ids + n, *old_len = counts + n;
  std::vector<uint64_t> ws;                                            // the plan as it goes up
  DrainOnExit drain{s};                                                // (the copies below write `hw`, the uploads read `ws`)
  ZRET(ingest_scan(d_counts, SPARSE_MAX_COUNT + 1, iw, s));
  hipLaunchKernelGGL(sparse_csr_check_kernel, dim3(ingest_wave_grid(n)), dim3(SPARSE_INGEST_THREADS), 0, s, d_counts, d_indices,
                     (const uint64_t *)iw.off, n, elements, iw.status);
  ZCHK(hipGetLastError());
  hipLaunchKernelGGL(sparse_put_lens_kernel, dim3((uint32_t)((n + SPARSE_PUT_THREADS - 1) / SPARSE_PUT_THREADS)), dim3(SPARSE_PUT_THREADS), 0, s,
                     (const uint64_t *)st.row_off, d_ids, n, old_n, h->put_ws.as<uint32_t>());
  ZCHK(hipGetLastError());
  ZCHK(hipMemcpyAsync(hw.data(), d_ids, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipMemcpyAsync(hw.data() + n, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipMemcpyAsync(hw.data() + 2 * n, h->put_ws.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  uint32_t status = 0;
  uint64_t total = 0;
  ZRET(ingest_read(iw, &status, &total, s));                           // the call's one wait
  if (status || total != elements) return ZVEC_HIP_ERR_INVALID_ARGUMENT;      // (nothing of the store has changed)
  bool ascending = true;
  for (uint64_t i = 0; i < n; ++i) {
    if (ids[i] == 0xffffffffu) return ZVEC_HIP_ERR_OUT_OF_RANGE;       // (kInvalidNodeId)
    if (i && ids[i] <= ids[i - 1]) ascending = false;
  }

  // the rows that remain: the last one of every id, ascending by id (keep[j] = its number in the call)
  std::vector<uint32_t> keep((size_t)n);
  for (uint64_t i = 0; i < n; ++i) keep[i] = (uint32_t)i;
  if (!ascending) {
    std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
    size_t o = 0;
    for (size_t i = 0; i < keep.size(); ++i)
      if (i + 1 == keep.size() || ids[keep[i + 1]] != ids[keep[i]]) keep[o++] = keep[i];      // (stable: the last of a run is the latest)
    keep.resize(o);
  }
  const uint32_t T = (uint32_t)keep.size();
  const uint64_t new_n = std::max<uint64_t>(old_n, (uint64_t)ids[keep.back()] + 1);
  if (new_n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  uint32_t m = 0;                                                      // overwritten rows: keep[0 .. m)
  while (m < T && ids[keep[m]] < old_n) ++m;

  // The device workspace, in 8-byte words, every part on a 16-byte boundary; the first four parts come from the host:
  //   tid[T] u32 | src[T] u32 | tval[T] | sb[T + 1] | tkey[T] | tbeg[m] | ds[2m + 3] | ss[2m + 2] | stage idx[S] u32 | stage val[S]
  auto even = [](uint64_t words) { return (words + 1) & ~1ull; };
  const uint64_t o_tid = 0, o_src = o_tid + even(((uint64_t)T + 1) / 2), o_tval = o_src + even(((uint64_t)T + 1) / 2), o_sb = o_tval + even(T),
                 o_tkey = o_sb + even((uint64_t)T + 1), up_words = o_tkey;
  ws.assign((size_t)up_words, 0);
  uint32_t *tid = reinterpret_cast<uint32_t *>(ws.data() + o_tid), *src = reinterpret_cast<uint32_t *>(ws.data() + o_src);
  int64_t *tval = reinterpret_cast<int64_t *>(ws.data() + o_tval);
  uint64_t *sb = ws.data() + o_sb;
  int64_t shift = 0;
  bool same = true;
  for (uint32_t j = 0; j < T; ++j) {
    tid[j] = ids[keep[j]];
    src[j] = keep[j];
    sb[j + 1] = sb[j] + counts[keep[j]];
    if (j < m) {
      const uint64_t nl = counts[keep[j]], ol = old_len[keep[j]];
      if (ol > SPARSE_MAX_COUNT) return ZVEC_HIP_ERR_RUNTIME;          // (the store's own offsets: never)
      same = same && nl == ol;
      shift += (int64_t)nl - (int64_t)ol;
      tval[j] = shift;
    }
  }
  const uint64_t S = sb[T];
  const uint64_t tail_base = old_elems + (uint64_t)shift, new_elems = tail_base + (S - sb[m]);
  for (uint32_t j = m; j < T; ++j) tval[j] = (int64_t)(tail_base + (sb[j + 1] - sb[m]));
  const uint64_t o_tbeg = o_tkey + even(T), o_ds = o_tbeg + even(m), o_ss = o_ds + even(2ull * m + 3), o_sidx = o_ss + even(2ull * m + 2),
                 o_sval = o_sidx + even((S + 1) / 2), ws_words = o_sval + even((S * width + 7) / 8);
  ZRET(h->put_ws.ensure((size_t)ws_words * 8));                        // (the old lengths have been read: the block may move)
  uint64_t *d_ws = h->put_ws.as<uint64_t>();
  const int route = m == 0 ? 0 : same ? 1 : 2;
  const uint64_t gap = (new_n - old_n) - (T - m);                      // holes the call leaves behind the old rows
  ZRET(w.cover(new_n, gap != 0));                                      // (the hole bits span the new rows before anything changes)

  const uint32_t *d_tid = reinterpret_cast<const uint32_t *>(d_ws + o_tid), *d_sidx = reinterpret_cast<const uint32_t *>(d_ws + o_sidx);
  const void *d_sval = d_ws + o_sval;
  // the plan goes up once every allocation of the route has succeeded; stage, keys and pieces are made from it where they are read
  auto build_ws = [&]() -> int {
    ZCHK(hipMemcpyAsync(d_ws, ws.data(), (size_t)up_words * 8, hipMemcpyHostToDevice, s));
    SparsePutStageArgs ga{reinterpret_cast<const uint32_t *>(d_ws + o_src), d_tid, d_ws + o_sb, iw.off, d_indices, d_values, d_keys, T,
                          reinterpret_cast<uint32_t *>(d_ws + o_sidx), d_ws + o_sval, d_ws + o_tkey};
    const uint32_t grid = std::min<uint32_t>((T + SPARSE_PUT_THREADS / 64 - 1) / (SPARSE_PUT_THREADS / 64), 2048);
    if (width == 2) hipLaunchKernelGGL((sparse_put_stage_kernel<uint16_t>), dim3(grid), dim3(SPARSE_PUT_THREADS), 0, s, ga);
    else hipLaunchKernelGGL((sparse_put_stage_kernel<uint32_t>), dim3(grid), dim3(SPARSE_PUT_THREADS), 0, s, ga);
    ZCHK(hipGetLastError());
    if (m) {
      SparsePutPiecesArgs pa{st.row_off, d_tid, reinterpret_cast<const int64_t *>(d_ws + o_tval), d_ws + o_sb, m, tail_base, new_elems,
                             d_ws + o_tbeg, d_ws + o_ds, d_ws + o_ss};
      hipLaunchKernelGGL(sparse_put_pieces_kernel, dim3(m / SPARSE_PUT_THREADS + 1), dim3(SPARSE_PUT_THREADS), 0, s, pa);
      ZCHK(hipGetLastError());
    }
    return 0;
  };
  SparsePutOffsetsArgs oa{};
  oa.tid = d_tid; oa.tkey = d_ws + o_tkey; oa.tval = reinterpret_cast<const int64_t *>(d_ws + o_tval);
  oa.old_n = old_n; oa.new_n = new_n; oa.tail_base = tail_base;
  auto launch_offsets = [&]() -> int {
    if (oa.r0 >= oa.new_n) return 0;
    const uint64_t grid = (oa.new_n - oa.r0 + SPARSE_PUT_THREADS - 1) / SPARSE_PUT_THREADS;
    hipLaunchKernelGGL(sparse_put_offsets_kernel, dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, oa);
    ZCHK(hipGetLastError());
    return 0;
  };
  uint64_t moved = 0;
  if (route != 2) {
    ZRET(st.reserve(new_n, new_elems, s));             // (no new length: new_elems = old_elems + the tail rows' pairs)
    ZRET(build_ws());
    if (m) {
      SparsePutRowsArgs ra{d_tid, d_ws + o_tkey, d_ws + o_tbeg, d_ws + o_sb, d_sidx, d_sval, st.idx, st.val, st.keys};
      if (width == 2) hipLaunchKernelGGL((sparse_put_rows_kernel<uint16_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      else hipLaunchKernelGGL((sparse_put_rows_kernel<uint32_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      ZCHK(hipGetLastError());
    }
    if (S > sb[m]) {                                   // the tail rows' pairs, behind the old ones
      ZCHK(hipMemcpyAsync(st.idx + old_elems, d_sidx + sb[m], (size_t)(S - sb[m]) * 4, hipMemcpyDeviceToDevice, s));
      ZCHK(hipMemcpyAsync(static_cast<char *>(st.val) + old_elems * width, static_cast<const char *>(d_sval) + sb[m] * width,
                          (size_t)(S - sb[m]) * width, hipMemcpyDeviceToDevice, s));
    }
    oa.tid += m; oa.tkey += m; oa.tval += m; oa.T = T - m; oa.m = 0; oa.r0 = old_n;
    oa.old_off = st.row_off; oa.old_keys = st.keys; oa.new_off = st.row_off; oa.new_keys = st.keys;
    ZRET(launch_offsets());
    ZCHK(hipStreamSynchronize(s));
    st.n = new_n;
    st.elems = new_elems;
    moved = S;
  } else {
    if ((new_elems + SPARSE_PUT_CHUNK - 1) / SPARSE_PUT_CHUNK > 0x7fffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (the splice's grid)
    uint64_t nr = 0, ne = 0;
    st.grown(new_n, new_elems, &nr, &ne);
    Scoped<uint64_t> n_off, n_keys;
    Scoped<uint32_t> n_idx;
    Scoped<void> n_val;
    ZRET(n_off.alloc((size_t)nr + 1));
    ZRET(n_keys.alloc((size_t)std::max<uint64_t>(nr, 1)));
    ZRET(n_idx.alloc((size_t)std::max<uint64_t>(ne, 1)));
    ZRET(n_val.alloc_bytes((size_t)std::max<uint64_t>(ne, 1) * width));
    ZRET(build_ws());
    if (new_elems) {
      SparsePutSpliceArgs sa{d_ws + o_ds, d_ws + o_ss, 2 * m + 2, new_elems, st.idx, d_sidx, st.val, d_sval, n_idx.p, n_val.p};
      const uint64_t grid = (new_elems + SPARSE_PUT_CHUNK - 1) / SPARSE_PUT_CHUNK;
      if (width == 2) hipLaunchKernelGGL((sparse_put_splice_kernel<uint16_t>), dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, sa);
      else hipLaunchKernelGGL((sparse_put_splice_kernel<uint32_t>), dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, sa);
      ZCHK(hipGetLastError());
    }
    oa.T = T; oa.m = m; oa.r0 = 0;
    oa.old_off = st.row_off; oa.old_keys = st.keys; oa.new_off = n_off.p; oa.new_keys = n_keys.p;
    ZRET(launch_offsets());
    ZCHK(hipStreamSynchronize(s));
    st.adopt(n_off, n_keys, n_idx, n_val, nr, ne, new_n, new_elems);      // (the old arrays go with the locals)
    moved = new_elems;
  }
  if (s != w.s) ZCHK(hipStreamSynchronize(w.s));       // (the hole bits grow on the handle's own stream)

  // the hole bits: the gaps between the old end and the call's tail rows are set, a written hole is cleared (no gap, no hole: no pass)
  uint64_t from = old_n;
  for (uint32_t j = m; j < T && gap; ++j) { h->holes.host.set_range(from, tid[j]); from = (uint64_t)tid[j] + 1; }
  for (uint32_t j = 0; j < m && h->holes.count(); ++j) h->holes.host.clear(tid[j]);
  h->put_route = route;
  h->put_moved = moved;
  const int e = w.finish();
  h->put_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return e;
}

}  // namespace
}  // extern "C++"

int zvec_hip_sparse_put_dev(zvec_hip_sparse_t h, const uint32_t *d_ids, const uint32_t *d_counts, const uint32_t *d_indices,
                            const void *d_values, uint64_t n, uint64_t elements, const uint64_t *d_keys, void *stream) {
  try {
    return sparse_put_dev(h, d_ids, d_counts, d_indices, d_values, n, elements, d_keys, stream);
  } catch (const std::bad_alloc &) {
    return ZVEC_HIP_ERR_NO_MEMORY;       // (a host table of the call: nothing of the store had changed yet)
  }
}
