// api_entry_sparse_put.inc.h — C ABI entry points: add-with-id on a sparse index (zvec_hip_sparse_put / _holes / _put_info; device side:
// zvk_sparse_put.hip.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// FlatSparseStreamerEntity::add_vector_with_id (flat_sparse_streamer_entity.cc:708-783) row by row: id == count appends, id > count
// pads [count, id) with empty rows under kInvalidKey first, id < count overwrites.  Applied in call order that leaves, for every
// position, the LAST row the call names for it, a hole where a gap was padded and never named, and everything else as it was; so the
// call is reduced to its rows sorted by id, the last of every id, and applied at once by one of three routes:
//   0 tail      every id is at or behind the old count: the append path plus empty rows for the gaps
//   1 in place  every overwritten row keeps its length: pairs and keys are written over the old ones (tail rows, if any, as route 0)
//   2 splice    an overwritten row changes its length: new idx / val / row_off / keys arrays are written whole by one pass over the
//               store and take the old ones' place (SparseStore::adopt), so no launch reads and writes the same array; until the
//               swap both copies of the arrays exist
// The old lengths of the overwritten rows come from a device gather of their offsets (two words a row and one wait): the host keeps
// no mirror of row_off, and nothing here grows with the store's row count.  Everything that can be refused or can run out of memory
// happens before the first byte of the store changes; the counts, the hole bits and put_info change last.

extern "C++" {
namespace {

// a stream is drained when the scope ends, however it ends: asynchronous copies out of pageable host memory declared BEFORE this
// object have left that memory by the time it is freed
struct DrainOnExit {
  hipStream_t s;
  ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};

// zvec_hip_sparse_put proper.  Every host allocation (and so every std::bad_alloc, which the entry turns into
// ZVEC_HIP_ERR_NO_MEMORY) comes before the first launch that writes the store.
int sparse_put(zvec_hip_sparse_s *h, const uint32_t *ids, const uint32_t *counts, const uint32_t *indices, const void *values, uint64_t n,
               const uint64_t *keys) {
  if (!h || (n && (!ids || !counts))) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  uint64_t total = 0;
  ZRET(sparse_check_runs(counts, indices, n, &total));       // (before anything is stored: a refused call stores nothing)
  if (total && (!indices || !values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  bool ascending = true;
  for (uint64_t i = 0; i < n; ++i) {
    if (ids[i] == 0xffffffffu) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (kInvalidNodeId)
    if (i && ids[i] <= ids[i - 1]) ascending = false;
  }
  const auto t0 = std::chrono::steady_clock::now();
  SparseWrite w(h);
  SparseStore &st = h->st;
  const uint32_t width = st.width;

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
  const uint64_t old_n = st.n, old_elems = st.elems;
  const uint64_t new_n = std::max<uint64_t>(old_n, (uint64_t)ids[keep.back()] + 1);
  if (new_n > 0xfffffffeull) return ZVEC_HIP_ERR_OUT_OF_RANGE;       // (positions are 32-bit in the partial lists, as in append)
  uint32_t m = 0;                                                    // overwritten rows: keep[0 .. m)
  while (m < T && ids[keep[m]] < old_n) ++m;
  std::vector<uint64_t> in_off((size_t)n + 1, 0);                    // where the call's runs start
  for (uint64_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + counts[i];
  std::vector<uint64_t> sb((size_t)T + 1, 0);                        // ... and where the kept ones start in the stage
  for (uint32_t j = 0; j < T; ++j) sb[j + 1] = sb[j] + counts[keep[j]];
  const uint64_t S = sb[T];

  ZRET(w.open());
  hipStream_t s = w.s;
  // The device workspace, in 8-byte words, every part on a 16-byte boundary:
  //   tid[T] u32 | gath[2m] | tkey[T] | tval[T] | tbeg[m] | sbeg[m + 1] | ds[2m + 3] | ss[2m + 2] | stage idx[S] u32 | stage val[S]
  auto even = [](uint64_t words) { return (words + 1) & ~1ull; };
  const uint64_t o_tid = 0, o_gath = o_tid + even(((uint64_t)T + 1) / 2), o_tkey = o_gath + even(2ull * m), o_tval = o_tkey + even(T),
                 o_tbeg = o_tval + even(T), o_sbeg = o_tbeg + even(m), o_ds = o_sbeg + even((uint64_t)m + 1),
                 o_ss = o_ds + even(2ull * m + 3), o_sidx = o_ss + even(2ull * m + 2), o_sval = o_sidx + even((S + 1) / 2),
                 ws_words = o_sval + even((S * width + 7) / 8);
  ZRET(h->put_ws.ensure((size_t)ws_words * 8));
  uint64_t *d_ws = h->put_ws.as<uint64_t>();
  std::vector<uint64_t> ws((size_t)ws_words, 0);
  DrainOnExit drain{s};                                              // (the uploads below read `ws`)
  uint32_t *tid = reinterpret_cast<uint32_t *>(ws.data() + o_tid);
  for (uint32_t j = 0; j < T; ++j) tid[j] = ids[keep[j]];
  // old begin and end of every overwritten row
  uint64_t *gath = ws.data() + o_gath;
  if (m) {
    ZCHK(hipMemcpyAsync(d_ws + o_tid, tid, (size_t)T * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sparse_put_gather_kernel, dim3((m + 255) / 256), dim3(256), 0, s, (const uint64_t *)st.row_off,
                       reinterpret_cast<const uint32_t *>(d_ws + o_tid), m, d_ws + o_gath);
    ZCHK(hipGetLastError());
    ZCHK(hipMemcpyAsync(gath, d_ws + o_gath, (size_t)m * 16, hipMemcpyDeviceToHost, s));
    ZCHK(hipStreamSynchronize(s));
  }
  // the tables: keys, shifts and ends, the pieces of the splice
  uint64_t *tkey = ws.data() + o_tkey, *tbeg = ws.data() + o_tbeg, *sbeg = ws.data() + o_sbeg, *ds = ws.data() + o_ds, *ss = ws.data() + o_ss;
  int64_t *tval = reinterpret_cast<int64_t *>(ws.data() + o_tval);
  int64_t shift = 0;
  bool same = true;
  for (uint32_t j = 0; j < m; ++j) {
    const uint64_t ob = gath[2 * (size_t)j], oe = gath[2 * (size_t)j + 1], nl = sb[j + 1] - sb[j];
    if (oe < ob || oe > old_elems) return ZVEC_HIP_ERR_RUNTIME;      // (the store's own offsets: never)
    ds[2 * (size_t)j] = j ? gath[2 * (size_t)j - 1] + (uint64_t)shift : 0;      // untouched segment j: from the previous row's old end
    ss[2 * (size_t)j] = j ? gath[2 * (size_t)j - 1] : 0;
    ds[2 * (size_t)j + 1] = ob + (uint64_t)shift;                                // new row j, from the stage
    ss[2 * (size_t)j + 1] = sb[j];
    same = same && nl == oe - ob;
    shift += (int64_t)nl - (int64_t)(oe - ob);
    tval[j] = shift;
    tbeg[j] = ob;
    sbeg[j] = sb[j];
  }
  sbeg[m] = sb[m];
  const uint64_t tail_base = old_elems + (uint64_t)shift, new_elems = tail_base + (S - sb[m]);
  if (m) {
    ds[2 * (size_t)m] = gath[2 * (size_t)m - 1] + (uint64_t)shift;    // the segment behind the last overwritten row
    ss[2 * (size_t)m] = gath[2 * (size_t)m - 1];
    ds[2 * (size_t)m + 1] = tail_base;                                // the call's tail rows, from the stage
    ss[2 * (size_t)m + 1] = sb[m];
    ds[2 * (size_t)m + 2] = new_elems;
  }
  for (uint32_t j = m; j < T; ++j) tval[j] = (int64_t)(tail_base + (sb[j + 1] - sb[m]));
  for (uint32_t j = 0; j < T; ++j) tkey[j] = keys ? keys[keep[j]] : (uint64_t)tid[j];
  uint32_t *sidx = reinterpret_cast<uint32_t *>(ws.data() + o_sidx);
  char *sval = reinterpret_cast<char *>(ws.data() + o_sval);
  for (uint32_t j = 0; j < T; ++j) {
    const uint64_t c = sb[j + 1] - sb[j], from = in_off[keep[j]];
    if (c == 0) continue;
    memcpy(sidx + sb[j], indices + from, (size_t)c * 4);
    memcpy(sval + sb[j] * width, static_cast<const char *>(values) + from * width, (size_t)c * width);
  }
  const int route = m == 0 ? 0 : same ? 1 : 2;
  const uint64_t gap = (new_n - old_n) - (T - m);                     // holes the call leaves behind the old rows
  ZRET(w.cover(new_n, gap != 0));                                     // (the hole bits span the new rows before anything changes)

  // the tables and the stage go up once every allocation of the route has succeeded (the ids are there already if they were gathered by)
  auto upload_ws = [&]() -> int {
    const uint64_t from = m ? o_tkey : 0;
    ZCHK(hipMemcpyAsync(d_ws + from, ws.data() + from, (size_t)(ws_words - from) * 8, hipMemcpyHostToDevice, s));
    return 0;
  };
  const uint32_t *d_tid = reinterpret_cast<const uint32_t *>(d_ws + o_tid), *d_sidx = reinterpret_cast<const uint32_t *>(d_ws + o_sidx);
  const void *d_sval = d_ws + o_sval;
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
    ZRET(st.reserve(new_n, new_elems, s));           // (no new length: new_elems = old_elems + the tail rows' pairs)
    ZRET(upload_ws());
    if (m) {
      SparsePutRowsArgs ra{d_tid, d_ws + o_tkey, d_ws + o_tbeg, d_ws + o_sbeg, d_sidx, d_sval, st.idx, st.val, st.keys};
      if (width == 2) hipLaunchKernelGGL((sparse_put_rows_kernel<uint16_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      else hipLaunchKernelGGL((sparse_put_rows_kernel<uint32_t>), dim3(m), dim3(SPARSE_PUT_THREADS), 0, s, ra);
      ZCHK(hipGetLastError());
    }
    if (S > sb[m]) {                                 // the tail rows' pairs, behind the old ones
      ZCHK(hipMemcpyAsync(st.idx + old_elems, d_sidx + sb[m], (size_t)(S - sb[m]) * 4, hipMemcpyDeviceToDevice, s));
      ZCHK(hipMemcpyAsync(static_cast<char *>(st.val) + old_elems * width, static_cast<const char *>(d_sval) + sb[m] * width,
                          (size_t)(S - sb[m]) * width, hipMemcpyDeviceToDevice, s));
    }
    // offsets and keys of the positions behind the old rows, in place: the table is the tail rows' alone
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
    ZRET(upload_ws());
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
