// api_entry_sparse_put.inc.h — C ABI entry points: add-with-id on a sparse index (zvec_hip_sparse_put / _holes / _put_info), and
// put_apply, the part of a put that zvec_hip_sparse_put_dev (api_entry_sparse_put_dev.inc.h) shares with it.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// What a put is, the keep-last rule and the three routes: host/sparse_put_plan.h, which also makes the plan of a call and lays out
// its workspace; the kernels: zvk_sparse_put.hip.h.  An entry brings the plan's inputs to the host — the ids, the counts and the old
// lengths of the rows the call overwrites, which come from the device (the host keeps no mirror of row_off, and nothing here grows
// with the store's row count) — and says how tables and stage get onto the device; put_apply does the rest.  Everything that can be
// refused or can run out of memory happens before the first byte of the store changes; the counts, the hole bits and put_info change
// last.

extern "C++" {
namespace {

// a stream is drained when the scope ends, however it ends: asynchronous copies out of (or into) pageable host memory declared
// BEFORE this object have left that memory by the time it is freed.  So in an entry: the vectors, then this, then the first copy.
struct DrainOnExit {
  hipStream_t s;
  ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};

// A planned put, applied.  L is placed (SparsePutLayout::place), tid is the plan's table on the host, t0 when the call began.
// fill(d_ws) gets the plan's tables, the kept rows' keys and the stage onto the device, into the workspace at d_ws on `s`; it is called
// once every allocation of the route has succeeded.
template <typename Fill>
int put_apply(SparseWrite &w, hipStream_t s, const SparsePutPlan &p, const SparsePutLayout &L, const uint32_t *tid,
              std::chrono::steady_clock::time_point t0, Fill fill) {
  zvec_hip_sparse_s *h = w.h;
  SparseStore &st = h->st;
  const uint32_t width = st.width, T = p.T, m = p.m;
  ZRET(h->put_ws.ensure((size_t)L.words * 8));
  uint64_t *d_ws = h->put_ws.as<uint64_t>();
  ZRET(w.cover(p.new_n, p.gap != 0));                                 // (the hole bits span the new rows before anything changes)

  const uint32_t *d_tid = reinterpret_cast<const uint32_t *>(d_ws + L.tid), *d_sidx = reinterpret_cast<const uint32_t *>(d_ws + L.sidx);
  const int64_t *d_tval = reinterpret_cast<const int64_t *>(d_ws + L.tval);
  const uint64_t *d_sb = d_ws + L.sb;
  const void *d_sval = d_ws + L.sval;
  // tables and stage, then for overwritten rows where they begin and the pieces of the splice, from the store's own offsets
  auto fill_ws = [&]() -> int {
    ZRET(fill(d_ws));
    if (m) {
      SparsePutPiecesArgs pa{st.row_off, d_tid, d_tval, d_sb, m, p.tail_base, p.new_elems, d_ws + L.tbeg, d_ws + L.ds, d_ws + L.ss};
      hipLaunchKernelGGL(sparse_put_pieces_kernel, dim3(m / SPARSE_PUT_THREADS + 1), dim3(SPARSE_PUT_THREADS), 0, s, pa);
      ZCHK(hipGetLastError());
    }
    return 0;
  };
  SparsePutOffsetsArgs oa{};
  oa.tid = d_tid; oa.tkey = d_ws + L.tkey; oa.tval = d_tval;
  oa.old_n = p.old_n; oa.new_n = p.new_n; oa.tail_base = p.tail_base;
  auto launch_offsets = [&]() -> int {
    if (oa.r0 >= oa.new_n) return 0;
    const uint64_t grid = (oa.new_n - oa.r0 + SPARSE_PUT_THREADS - 1) / SPARSE_PUT_THREADS;
    hipLaunchKernelGGL(sparse_put_offsets_kernel, dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, oa);
    ZCHK(hipGetLastError());
    return 0;
  };
  uint64_t moved = 0;
  if (p.route != 2) {
    ZRET(st.reserve(p.new_n, p.new_elems, s));       // (no new length: new_elems = old_elems + the tail rows' pairs)
    ZRET(fill_ws());
    if (m) {
      SparsePutRowsArgs ra{d_tid, d_ws + L.tkey, d_ws + L.tbeg, d_sb, d_sidx, d_sval, st.idx, st.val, st.keys};
      if (width == 2) hipLaunchKernelGGL((sparse_put_rows_kernel<uint16_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      else hipLaunchKernelGGL((sparse_put_rows_kernel<uint32_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      ZCHK(hipGetLastError());
    }
    if (p.S > p.S_over) {                            // the tail rows' pairs, behind the old ones
      ZCHK(hipMemcpyAsync(st.idx + p.old_elems, d_sidx + p.S_over, (size_t)(p.S - p.S_over) * 4, hipMemcpyDeviceToDevice, s));
      ZCHK(hipMemcpyAsync(static_cast<char *>(st.val) + p.old_elems * width, static_cast<const char *>(d_sval) + p.S_over * width,
                          (size_t)(p.S - p.S_over) * width, hipMemcpyDeviceToDevice, s));
    }
    // offsets and keys of the positions behind the old rows, in place: the table is the tail rows' alone
    oa.tid += m; oa.tkey += m; oa.tval += m; oa.T = T - m; oa.m = 0; oa.r0 = p.old_n;
    oa.old_off = st.row_off; oa.old_keys = st.keys; oa.new_off = st.row_off; oa.new_keys = st.keys;
    ZRET(launch_offsets());
    ZCHK(hipStreamSynchronize(s));
    st.n = p.new_n;
    st.elems = p.new_elems;
    moved = p.S;
  } else {
    uint64_t nr = 0, ne = 0;
    st.grown(p.new_n, p.new_elems, &nr, &ne);
    Scoped<uint64_t> n_off, n_keys;
    Scoped<uint32_t> n_idx;
    Scoped<void> n_val;
    ZRET(n_off.alloc((size_t)nr + 1));
    ZRET(n_keys.alloc((size_t)std::max<uint64_t>(nr, 1)));
    ZRET(n_idx.alloc((size_t)std::max<uint64_t>(ne, 1)));
    ZRET(n_val.alloc_bytes((size_t)std::max<uint64_t>(ne, 1) * width));
    ZRET(fill_ws());
    if (p.new_elems) {
      SparsePutSpliceArgs sa{d_ws + L.ds, d_ws + L.ss, 2 * m + 2, p.new_elems, st.idx, d_sidx, st.val, d_sval, n_idx.p, n_val.p};
      const uint64_t grid = (p.new_elems + SPARSE_PUT_CHUNK - 1) / SPARSE_PUT_CHUNK;      // (in range: put_plan)
      if (width == 2) hipLaunchKernelGGL((sparse_put_splice_kernel<uint16_t>), dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, sa);
      else hipLaunchKernelGGL((sparse_put_splice_kernel<uint32_t>), dim3((uint32_t)grid), dim3(SPARSE_PUT_THREADS), 0, s, sa);
      ZCHK(hipGetLastError());
    }
    oa.T = T; oa.m = m; oa.r0 = 0;
    oa.old_off = st.row_off; oa.old_keys = st.keys; oa.new_off = n_off.p; oa.new_keys = n_keys.p;
    ZRET(launch_offsets());
    ZCHK(hipStreamSynchronize(s));
    st.adopt(n_off, n_keys, n_idx, n_val, nr, ne, p.new_n, p.new_elems);      // (the old arrays go with the locals)
    moved = p.new_elems;
  }
  if (s != w.s) ZCHK(hipStreamSynchronize(w.s));     // (a caller's stream: the hole bits grow on the handle's own)

  put_holes(h->holes.host, p, tid);
  h->put_route = p.route;
  h->put_moved = moved;
  const int e = w.finish();
  h->put_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return e;
}

// zvec_hip_sparse_put proper: the call's rows in host memory.  The run check, the staging of the kept rows' pairs and their keys are
// the host's; the old lengths of the call's rows come back from sparse_put_lens_kernel in a wait of their own (4 bytes a row), which a
// call that overwrites nothing skips.  Every host allocation (and so every std::bad_alloc, which the entry turns into
// ZVEC_HIP_ERR_NO_MEMORY) comes before the first launch that writes the store.
int sparse_put(zvec_hip_sparse_s *h, const uint32_t *ids, const uint32_t *counts, const uint32_t *indices, const void *values, uint64_t n,
               const uint64_t *keys) {
  if (!h || (n && (!ids || !counts))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  uint64_t total = 0;
  ZRET(sparse_check_runs(counts, indices, n, &total));       // (before anything is stored: a refused call stores nothing)
  if (total && (!indices || !values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> keep;
  ZRET(put_keep(ids, n, keep));
  SparseWrite w(h);
  SparseStore &st = h->st;
  const uint32_t width = st.width;
  ZRET(w.open());
  hipStream_t s = w.s;

  std::vector<uint32_t> old_len;                                     // of the call's rows
  std::vector<uint64_t> ws;                                          // the workspace as it goes up
  DrainOnExit drain{s};                                              // (the copies below write `old_len` and read `ws`)
  if (ids[keep[0]] < st.n) {                                         // some row is overwritten (the kept ids ascend)
    old_len.resize((size_t)n);
    // ids | old lengths, read back below; with room for the whole workspace (m <= T, S <= total), so that put_apply's ensure finds
    // it there and a call allocates once
    SparsePutLayout room((uint32_t)keep.size());
    room.place((uint32_t)keep.size(), total, width);
    ZRET(h->put_ws.ensure((size_t)std::max<uint64_t>(room.words, n) * 8));
    uint32_t *d_ids = h->put_ws.as<uint32_t>();
    ZCHK(hipMemcpyAsync(d_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sparse_put_lens_kernel, dim3((uint32_t)((n + SPARSE_PUT_THREADS - 1) / SPARSE_PUT_THREADS)), dim3(SPARSE_PUT_THREADS), 0, s,
                       (const uint64_t *)st.row_off, (const uint32_t *)d_ids, n, st.n, d_ids + n);
    ZCHK(hipGetLastError());
    ZCHK(hipMemcpyAsync(old_len.data(), d_ids + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    ZCHK(hipStreamSynchronize(s));
  }
  SparsePutLayout L((uint32_t)keep.size());
  ws.assign((size_t)L.tkey, 0);
  SparsePutPlan p;
  ZRET(put_plan(p, keep, ids, counts, old_len.data(), st.n, st.elems, SPARSE_MAX_COUNT, SPARSE_PUT_CHUNK, L, ws.data()));
  L.place(p.m, p.S, width);
  ws.resize((size_t)L.words, 0);                                     // (nothing has been copied out of it yet)

  // the keys and the stage: the kept rows' pairs back to back
  std::vector<uint64_t> in_off((size_t)n + 1, 0);                    // where the call's runs start
  for (uint64_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + counts[i];
  const uint32_t *tid = reinterpret_cast<const uint32_t *>(ws.data() + L.tid);
  const uint64_t *sb = ws.data() + L.sb;
  uint64_t *tkey = ws.data() + L.tkey;
  uint32_t *sidx = reinterpret_cast<uint32_t *>(ws.data() + L.sidx);
  char *sval = reinterpret_cast<char *>(ws.data() + L.sval);
  for (uint32_t j = 0; j < p.T; ++j) {
    const uint64_t c = sb[j + 1] - sb[j], from = in_off[keep[j]];
    tkey[j] = keys ? keys[keep[j]] : (uint64_t)tid[j];
    if (c == 0) continue;
    memcpy(sidx + sb[j], indices + from, (size_t)c * 4);
    memcpy(sval + sb[j] * width, static_cast<const char *>(values) + from * width, (size_t)c * width);
  }
  return put_apply(w, s, p, L, tid, t0, [&](uint64_t *d_ws) -> int {
    ZCHK(hipMemcpyAsync(d_ws, ws.data(), (size_t)L.words * 8, hipMemcpyHostToDevice, s));
    return 0;
  });
}

}  // namespace
}  // extern "C++"

int zvec_hip_sparse_put(zvec_hip_sparse_t h, const uint32_t *ids, const uint32_t *counts, const uint32_t *indices, const void *values,
                        uint64_t n, const uint64_t *keys) {
  try {
    return sparse_put(h, ids, counts, indices, values, n, keys);
  } catch (const std::bad_alloc &) {
    return ZVEC_HIP_ERR_NO_MEMORY;       // (a host table of the call: nothing of the store had changed yet)
  }
}

int zvec_hip_sparse_holes(zvec_hip_sparse_t h, uint64_t *count) {
  if (!h || !count) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  *count = h->holes.count();
  return 0;
}

int zvec_hip_sparse_put_info(zvec_hip_sparse_t h, int *route, uint64_t *moved_elems, uint32_t *chunk_elems, double *ms) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (route) *route = h->put_route;
  if (moved_elems) *moved_elems = h->put_moved;
  if (chunk_elems) *chunk_elems = SPARSE_PUT_CHUNK;
  if (ms) *ms = h->put_ms;
  return 0;
}
