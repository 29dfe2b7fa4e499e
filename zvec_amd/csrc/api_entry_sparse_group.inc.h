// api_entry_sparse_group.inc.h — C ABI entry points: group-by search over sparse rows (inside extern "C")
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).
//
// FlatSparseSearcher / FlatSparseStreamer with group parameters set (the dispatch, flat_sparse_search.h:77-117):
// FlatSparseEntity::search_group and search_group_p_keys (flat_sparse_entity.h:79-128) keep one bounded heap of `group_topk`
// documents per group id while they walk the rows (or the listed keys), ConvertGroupMapToResult (flat_sparse_search.h:23-53)
// orders the groups by their best score, keeps the first `group_num` and cuts every list at the radius.  Here the scores of a
// batch are a candidate matrix in HBM and group_select (api_entry_group.inc.h) does the selection, as for the dense flat index:
//   full scan    [queries][n] scores, no index matrix; a sub-batch of at most "sparse_group_rows" queries is dumped by
//                sparse_rows_dump_kernel (a wave per stored row: zvec calls once per query), a wider one by
//                sparse_scan_kernel<.., DUMP = true> (lane = query)
//   listed rows  sparse_rows_kernel with a row stride: [queries][longest list] scores and positions, +inf / IDX_NONE for padding
//                and for skipped entries
// The scores are final as they stand (minus the inner product, or the squared distance A + R of an L2 handle): nothing is refined.

}  // extern "C"

namespace {

template <typename VT, bool L2>
int launch_sparse_rows_dump(const SparseRowsDumpArgs &a, uint32_t grid, size_t lds, hipStream_t stream) {
  // (indices | values of one run: at most 32 KiB, no launch attribute needed)
  if (a.op.exclude) hipLaunchKernelGGL((sparse_rows_dump_kernel<VT, true, L2>), dim3(grid), dim3(64), lds, stream, a);
  else hipLaunchKernelGGL((sparse_rows_dump_kernel<VT, false, L2>), dim3(grid), dim3(64), lds, stream, a);
  ZCHK(hipGetLastError());
  return 0;
}

// what the two entry points check alike before count == 0 returns 0; *total = the queries' pairs
int sparse_group_args_ok(zvec_hip_sparse_t h, const uint32_t *q_counts, const uint32_t *q_indices, const void *q_values, uint32_t count,
                         const uint32_t *group_of_position, uint32_t ngroups, uint32_t gnum, uint32_t gk, const uint32_t *out_groups,
                         const uint32_t *out_ngroups, const uint64_t *out_keys, const float *out_scores, const uint32_t *out_counts,
                         uint64_t *total) {
  if (!h || !group_of_position || !out_groups || !out_ngroups || !out_keys || !out_scores || !out_counts || (count && !q_counts))
    return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZRET(group_args_ok(ngroups, gnum, gk));
  return sparse_queries_ok(q_counts, q_indices, q_values, count, 0, total);
}

// an empty index: no groups (and nothing stale in the caller's arrays)
int sparse_group_empty(zvec_hip_ctx_s *c, const GroupOut &o, uint32_t count, uint32_t gnum, uint32_t gk, hipStream_t s) {
  const size_t rows = (size_t)count * gnum;
  ZCHK(hipMemsetAsync(o.ngroups, 0, (size_t)count * 4, s));
  ZCHK(hipMemsetAsync(o.counts, 0, rows * 4, s));
  ZCHK(hipMemsetAsync(o.groups, 0xff, rows * 4, s));
  ZCHK(hipMemsetAsync(o.keys, 0xff, rows * gk * 8, s));
  ZCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(o.scores), 0x7f800000, rows * gk, s));
  return 0;
}

}  // namespace

extern "C" {

int zvec_hip_sparse_search_grouped(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                                   const void *q_values, uint32_t count, const uint32_t *group_of_position, uint32_t ngroups,
                                   uint32_t group_num, uint32_t group_topk, float threshold, const uint64_t *exclude_bitset,
                                   uint32_t *out_groups, uint32_t *out_ngroups, uint64_t *out_keys, float *out_scores,
                                   uint32_t *out_counts) {
  uint64_t total = 0;
  ZRET(sparse_group_args_ok(h, q_counts, q_indices, q_values, count, group_of_position, ngroups, group_num, group_topk, out_groups,
                            out_ngroups, out_keys, out_scores, out_counts, &total));
  if (count == 0) return 0;
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->st.width, total, q_indices, q_values, blob, &te);      // (the width never changes after create)
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);          // the row count the bitset and group_of_position are sized for == the rows scanned
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = c->cur;
  const SparseStore &st = h->st;
  GroupOut o{};
  ZRET(group_outputs(c, count, group_num, group_topk, &o));
  if (st.n == 0) {
    ZRET(sparse_group_empty(c, o, count, group_num, group_topk, s));
    return group_copy_out(c, o, count, group_num, group_topk, out_groups, out_ngroups, out_keys, out_scores, out_counts, s);
  }
  ZRET(c->grp_of.ensure((size_t)st.n * 4));
  ZCHK(hipMemcpyAsync(c->grp_of.p, group_of_position, (size_t)st.n * 4, hipMemcpyHostToDevice, s));
  ZRET(host_search_wrap_begin(c, blob.data(), blob.size() * 4, exclude_bitset, st.n, count, 1, s));
  const uint32_t *dq = static_cast<const uint32_t *>(c->io_qp);
  // query slices: the score matrix stays <= 1 GiB, and a slice is one grid dimension of group_best_kernel (<= 65535)
  const uint32_t sub = dense_sub_batch(std::min<uint32_t>(count, 32768), st.n);
  std::vector<uint32_t> plan;
  uint32_t nblocks = 0, max_img = 0, max_run = 0;
  sparse_make_plan(q_counts, count, sub, plan, &nblocks, &max_img);          // q_off[count + 1] | blk[blocks + 1]
  for (uint32_t q = 0; q < count; ++q) max_run = std::max(max_run, q_counts[q]);
  ZRET(sparse_upload_plan(c, plan, s));
  ZRET(c->part_s.ensure((size_t)sub * st.n * 4));
  float *dump = c->part_s.as<float>();
  const uint64_t *d_ex = exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr;
  ZRET(effective_exclude(h->holes, st.n, c, d_ex, s, &d_ex));
  const SparseOperands op = sparse_operands(st, d_ex, c->sp_plan.as<uint32_t>(), dq, dq + te);
  const uint32_t wave_rows = (uint32_t)ropts().sparse_group_rows.load(std::memory_order_relaxed);
  for (uint32_t q0 = 0; q0 < count; q0 += sub) {
    const uint32_t cnt = std::min(sub, count - q0);
    if (cnt <= wave_rows) {
      // a wave per stored row: 16 one-wave work-groups per CU, a chunk is whole 64-row stores
      SparseRowsDumpArgs a{};
      a.op = op; a.qsub0 = q0; a.nqsub = cnt; a.n = st.n; a.dump = dump;
      const uint64_t want = std::max<uint64_t>(1, ((uint64_t)device_cus(c) * 16 + cnt - 1) / cnt);
      a.rows_per_chunk = (uint32_t)std::min<uint64_t>((((st.n + want - 1) / want + 63) / 64) * 64, 0x7fffffc0u);
      const uint32_t nchunks = (uint32_t)((st.n + a.rows_per_chunk - 1) / a.rows_per_chunk);
      ZRET(sparse_dispatch(st.width, h->l2(), [&](auto vt, auto l2) {
        return launch_sparse_rows_dump<decltype(vt), decltype(l2)::value>(a, nchunks * cnt, sparse_run_lds_bytes(max_run, st.width), s);
      }));
    } else {
      ZRET(sparse_dump_scores(h, c, op, plan, count, max_img, q0, cnt, dump, s));
    }
    ZRET(group_select(c, st.keys, nullptr, dump, nullptr, (uint32_t)st.n, (uint32_t)st.n, q0, cnt, c->grp_of.as<uint32_t>(), ngroups,
                      group_num, group_topk, threshold, o, s));
  }
  return group_copy_out(c, o, count, group_num, group_topk, out_groups, out_ngroups, out_keys, out_scores, out_counts, s);
}

int zvec_hip_sparse_search_grouped_by_ids(zvec_hip_sparse_t h, zvec_hip_ctx_t ctx, const uint32_t *q_counts, const uint32_t *q_indices,
                                          const void *q_values, uint32_t count, const uint32_t *ids, const uint32_t *offsets,
                                          const uint32_t *group_of_position, uint32_t ngroups, uint32_t group_num, uint32_t group_topk,
                                          float threshold, const uint64_t *exclude_bitset, uint32_t *out_groups, uint32_t *out_ngroups,
                                          uint64_t *out_keys, float *out_scores, uint32_t *out_counts) {
  uint64_t total = 0;
  ZRET(sparse_group_args_ok(h, q_counts, q_indices, q_values, count, group_of_position, ngroups, group_num, group_topk, out_groups,
                            out_ngroups, out_keys, out_scores, out_counts, &total));
  if (count == 0) return 0;
  uint32_t maxlen = 0;
  ZRET(sparse_lists_ok(ids, offsets, count, &maxlen));
  if ((uint64_t)count * maxlen > 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;      // (cells of the candidate matrix)
  size_t te = 0;
  std::vector<uint32_t> blob;
  sparse_stage_blob(h->st.width, total, q_indices, q_values, blob, &te);
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);          // the row count the bitset is sized for == the rows the positions are checked against
  ZCHK(hipSetDevice(h->device));
  hipStream_t s = c->cur;
  const SparseStore &st = h->st;
  GroupOut o{};
  ZRET(group_outputs(c, count, group_num, group_topk, &o));
  if (st.n == 0) {                                       // (every position is beyond the rows)
    ZRET(sparse_group_empty(c, o, count, group_num, group_topk, s));
    return group_copy_out(c, o, count, group_num, group_topk, out_groups, out_ngroups, out_keys, out_scores, out_counts, s);
  }
  ZRET(c->grp_of.ensure((size_t)st.n * 4));
  ZCHK(hipMemcpyAsync(c->grp_of.p, group_of_position, (size_t)st.n * 4, hipMemcpyHostToDevice, s));
  ZRET(host_search_wrap_begin(c, blob.data(), blob.size() * 4, exclude_bitset, st.n, count, 1, s));
  const uint32_t *dq = static_cast<const uint32_t *>(c->io_qp);
  const uint32_t *d_off = nullptr;
  ZRET(sparse_rows_locked(h, c, q_counts, dq, dq + te, count, ids, offsets, exclude_bitset ? c->io_ex.as<uint64_t>() : nullptr, &d_off, s,
                          maxlen));
  for (uint32_t q0 = 0; q0 < count; q0 += 32768)       // (a slice is one grid dimension of group_best_kernel)
    ZRET(group_select(c, st.keys, nullptr, c->part_s.as<float>() + (size_t)q0 * maxlen, c->part_i.as<uint32_t>() + (size_t)q0 * maxlen,
                      maxlen, maxlen, q0, std::min<uint32_t>(32768, count - q0), c->grp_of.as<uint32_t>(), ngroups, group_num, group_topk,
                      threshold, o, s));
  return group_copy_out(c, o, count, group_num, group_topk, out_groups, out_ngroups, out_keys, out_scores, out_counts, s);
}
