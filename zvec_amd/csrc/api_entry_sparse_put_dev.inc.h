// api_entry_sparse_put_dev.inc.h — C ABI entry point: add-with-id on a sparse index with the call's rows in device memory
// (zvec_hip_sparse_put_dev; device side: zvk_sparse_put.hip.h, the checks of zvk_sparse_ingest.hip.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// zvec_hip_sparse_put with the host's share of the pairs taken away.  What that entry does on the host with the pairs — the run check
// and the stage — is done on the device here, by the scan and check of zvec_hip_sparse_append_dev and by sparse_put_stage_kernel; what
// takes one word a row stays on the host (host/sparse_put_plan.h).  So
//   scan of d_counts -> sparse_csr_check_kernel -> sparse_put_lens_kernel (the old lengths at the call's ids)
//   ONE wait: the status word, the total, and per row its id, its count and its old length (12 bytes a row)
//   keep and plan on the host -> put_apply (api_entry_sparse_put.inc.h), whose fill is: the plan goes up (tid, src, tval, sb: 24 bytes
//   a kept row) -> sparse_put_stage_kernel (stage and keys).
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
  ZRET(w.open());
  hipStream_t s = stream ? reinterpret_cast<hipStream_t>(stream) : w.s;

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
                     (const uint64_t *)st.row_off, d_ids, n, st.n, h->put_ws.as<uint32_t>());
  ZCHK(hipGetLastError());
  ZCHK(hipMemcpyAsync(hw.data(), d_ids, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipMemcpyAsync(hw.data() + n, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  ZCHK(hipMemcpyAsync(hw.data() + 2 * n, h->put_ws.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  uint32_t status = 0;
  uint64_t total = 0;
  ZRET(ingest_read(iw, &status, &total, s));                           // the call's one wait
  if (status || total != elements) return ZVEC_HIP_ERR_INVALID_ARGUMENT;      // (nothing of the store has changed)
  std::vector<uint32_t> keep;
  ZRET(put_keep(ids, n, keep));
  SparsePutLayout L((uint32_t)keep.size());
  ws.assign((size_t)L.tkey, 0);
  SparsePutPlan p;
  ZRET(put_plan(p, keep, ids, counts, old_len, st.n, st.elems, SPARSE_MAX_COUNT, SPARSE_PUT_CHUNK, L, ws.data()));
  L.place(p.m, p.S, st.width);
  // (put_apply may move put_ws: the old lengths have been read)
  return put_apply(w, s, p, L, reinterpret_cast<const uint32_t *>(ws.data() + L.tid), t0, [&](uint64_t *d_ws) -> int {
    ZCHK(hipMemcpyAsync(d_ws, ws.data(), (size_t)L.tkey * 8, hipMemcpyHostToDevice, s));
    SparsePutStageArgs ga{reinterpret_cast<const uint32_t *>(d_ws + L.src), reinterpret_cast<const uint32_t *>(d_ws + L.tid), d_ws + L.sb, iw.off,
                          d_indices, d_values, d_keys, p.T, reinterpret_cast<uint32_t *>(d_ws + L.sidx), d_ws + L.sval, d_ws + L.tkey};
    const uint32_t grid = std::min<uint32_t>((p.T + SPARSE_PUT_THREADS / 64 - 1) / (SPARSE_PUT_THREADS / 64), 2048);
    if (st.width == 2) hipLaunchKernelGGL((sparse_put_stage_kernel<uint16_t>), dim3(grid), dim3(SPARSE_PUT_THREADS), 0, s, ga);
    else hipLaunchKernelGGL((sparse_put_stage_kernel<uint32_t>), dim3(grid), dim3(SPARSE_PUT_THREADS), 0, s, ga);
    ZCHK(hipGetLastError());
    return 0;
  });
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
