// api_entry_hnsw_sparse_build.inc.h — C ABI entry points: building an HNSW graph over SPARSE rows on the device
// (zvec_hip_hnsw_sparse_build*; inside extern "C").  Device code: the build kernels of zvk_hnsw_build.hip.h on the model of
// zvk_hnsw_sparse.hip.h.  Stands behind HnswSparseBuilder (src/core/algorithm/hnsw_sparse/hnsw_sparse_builder.cc).  The rule is
// DESIGN §3c "Building" unchanged, and so is the host's share: the plan (hnsw_plan_call, host/hnsw_add_plan.h), the rounds' scratch
// and the rounds themselves (HnswRoundsScratch, hnsw_rounds_of of api_entry_hnsw_build.inc.h).  Runs in, searchable graph out: the
// handle of api_entry_hnsw_sparse.inc.h then answers search, info, get_vector and export as after a load.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// A build is an insertion from base 0 into a fresh graph over fresh rows; both take the old ones' place on success.  Everything that
// can be refused is refused, and everything that is allocated is allocated, on locals: a refused build leaves the handle as it was.
static int hnsw_sparse_build_entry(zvec_hip_hnsw_sparse_t h, uint64_t n, const uint32_t *counts, const uint32_t *indices, const void *values,
                                   bool on_device, const uint64_t *keys, const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h || (n && !counts)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  uint64_t total = 0;
  if (n) ZRET(sparse_check_runs(counts, on_device ? nullptr : indices, n, &total));      // (device pairs: ascending is the caller's contract)
  if (total && (!indices || !values)) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  HnswWriteOf<zvec_hip_hnsw_sparse_s> w(h);
  ZRET(w.open());
  HnswInsertPlan pl;
  ZRET(hnsw_plan_call(HnswShape(), nullptr, false, n, counts, p, levels, pl));
  ZRET(w.quiesce());
  HnswGraph g;
  HnswSparseRows rows;
  HnswRoundsScratch ws;
  HnswInsertDone done;
  bool grew_rows, grew_upper;
  ZRET(ws.prepare(h->defctx, pl));
  ZRET(g.resize(pl.after, 0, h->defctx->cur, grew_rows, grew_upper));      // (lists and counts zero, upper_of IDX_NONE)
  ZRET(g.put_keys(0, n, keys));
  ZRET(rows.put(counts, n, total, indices, values, h->width, on_device));
  if (pl.after.stride) ZCHK(hipMemcpy(g.arr.upper_of.p, pl.upper_of.data(), (size_t)pl.count * 4, hipMemcpyHostToDevice));
  ZCHK(hipDeviceSynchronize());                  // (a device-to-device copy of pairs may still be in flight on the null stream)
  const uint32_t longest = n ? *std::max_element(counts, counts + n) : 0u;
  ZRET(sparse_dispatch(h->width, [&](auto vt) -> int {     // (both slots of a wave are sized by the longest row)
    const HnswCsrRows<decltype(vt)> model{SparseOperands{rows.row_off, rows.idx, rows.val, nullptr, nullptr, nullptr, nullptr}, longest};
    return hnsw_rounds_of(h->defctx, g.args(0, 0, ZVEC_HIP_METRIC_IP), model, g, pl, ws, done);
  }));
  hnsw_insert_finish(g, pl, done);
  hnsw_sparse_commit(h, g, rows);                // the old arrays go with the locals
  h->params = pl.q;
  h->built = true;
  h->bdone = done;
  return 0;
}

// HnswSparseBuilder::train + build: every row goes through HnswSparseAlgorithm::add_node
int zvec_hip_hnsw_sparse_build(zvec_hip_hnsw_sparse_t h, uint64_t n, const uint32_t *counts, const uint32_t *indices, const void *values,
                               const uint64_t *keys, const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  return hnsw_sparse_build_entry(h, n, counts, indices, values, false, keys, p, levels);
}

// the same with the pairs in device memory already; counts, keys and levels stay host arrays
int zvec_hip_hnsw_sparse_build_dev(zvec_hip_hnsw_sparse_t h, uint64_t n, const uint32_t *counts, const uint32_t *d_indices,
                                   const void *d_values, const uint64_t *keys, const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  return hnsw_sparse_build_entry(h, n, counts, d_indices, d_values, true, keys, p, levels);
}

int zvec_hip_hnsw_sparse_last_build_info(zvec_hip_hnsw_sparse_t h, zvec_hip_hnsw_build_info *out) {
  if (!h || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->built) return ZVEC_HIP_ERR_NO_READY;
  *out = zvec_hip_hnsw_build_info();
  hnsw_info_common(*out, h->bdone);
  return 0;
}
