// api_entry_hnsw_group.inc.h — C ABI entry points: group-by search on a built HNSW graph of dense rows (zvec_hip_hnsw_search_grouped*;
// inside extern "C").  Device code: zvk_hnsw_group.hip.h.  The rule is "Group-by" of DESIGN §3c: HnswAlgorithm::search with
// expand_neighbors_by_group (hnsw_algorithm.cc:102-104, 280-392) and HnswContext::topk_to_group_result (hnsw_context.h:188-250).
// Slicing, the workspace and the record of the last search are hnsw_search_sliced's, as for zvec_hip_hnsw_search; the outputs are
// those of zvec_hip_flat_search_grouped (group_outputs / group_copy_out, api_entry_group.inc.h).
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// what both entries refuse before they touch anything
static int hnsw_group_args(const void *h, const void *queries, uint32_t group_num, uint32_t group_topk, uint32_t ef, const GroupOut &o) {
  if (!h || !queries || !o.groups || !o.ngroups || !o.keys || !o.scores || !o.counts) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (group_num == 0 || group_topk == 0) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  return ef > HNSW_MAX_EF || (uint64_t)group_num * group_topk > HNSW_MAX_EF ? ZVEC_HIP_ERR_UNSUPPORTED : 0;
}

// the caller holds c->mu and h->rw (shared) and has validated the arguments; d_group_of is not read when the graph has no nodes
static int hnsw_group_search_dev_locked(zvec_hip_hnsw_s *h, zvec_hip_ctx_s *c, const void *d_queries, uint32_t count,
                                        const uint32_t *d_group_of, uint32_t ngroups, uint32_t gnum, uint32_t gk, uint32_t ef,
                                        uint32_t max_scan, float threshold, const uint64_t *d_exclude, const GroupOut &o, hipStream_t s) {
  HnswGroupArgs ga{d_group_of, ngroups, gnum, gk, nullptr, nullptr};
  // (as a plain search of topk = gnum * gk documents a query: ef_eff = max(ef, topk), and keys and scores are sliced by that many)
  ZRET(hnsw_search_sliced(h, h->graph, h->graph.args(h->dim, h->dpad, h->metric), c, count, gnum * gk, ef, max_scan, threshold, d_exclude,
                          o.keys, o.scores, o.counts, s, [&](HnswArgs &a, uint32_t q0, uint32_t mq) -> int {
    a.queries = static_cast<const unsigned char *>(d_queries) + (size_t)q0 * h->row_bytes();
    a.out_counts = o.counts + (size_t)q0 * gnum;
    ga.out_groups = o.groups + (size_t)q0 * gnum;
    ga.out_ngroups = o.ngroups + q0;
    return hnsw_with_rows(h, [&](auto rows) -> int {
      hipLaunchKernelGGL(hnsw_group_search_kernel<decltype(rows)::KIND>, dim3(mq), dim3(64),
                         hnsw_group_lds_bytes(hnsw_search_lds_bytes(rows.slot_bytes(a), a.ef, 0), gnum, gk), s, a, ga);
      ZCHK(hipGetLastError());
      return 0;
    });
  }));
  if (h->graph.n == 0) {
    ga.out_groups = o.groups; ga.out_ngroups = o.ngroups;
    hipLaunchKernelGGL(hnsw_group_empty_kernel, dim3((uint32_t)(((uint64_t)count * gnum + 255) / 256)), dim3(256), 0, s, ga, o.counts, count);
    ZCHK(hipGetLastError());
  }
  return 0;
}

int zvec_hip_hnsw_search_grouped_dev(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *d_queries, uint32_t count,
                                     const uint32_t *d_group_of_node, uint32_t ngroups, uint32_t group_num, uint32_t group_topk,
                                     uint32_t ef, uint32_t max_scan, float threshold, const uint64_t *d_exclude_bitset,
                                     uint32_t *d_out_groups, uint32_t *d_out_ngroups, uint64_t *d_out_keys, float *d_out_scores,
                                     uint32_t *d_out_counts, void *stream) {
  const GroupOut o{d_out_groups, d_out_ngroups, d_out_keys, d_out_scores, d_out_counts};
  ZRET(hnsw_group_args(h, d_queries, group_num, group_topk, ef, o));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
  if (h->graph.n && !d_group_of_node) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  ZCHK(hipSetDevice(h->device));
  return hnsw_group_search_dev_locked(h, c, d_queries, count, d_group_of_node, ngroups, group_num, group_topk, ef, max_scan, threshold,
                                      d_exclude_bitset, o, pick_stream(c, stream));
}

int zvec_hip_hnsw_search_grouped(zvec_hip_hnsw_t h, zvec_hip_ctx_t ctx, const void *queries, uint32_t count, const uint32_t *group_of_node,
                                 uint32_t ngroups, uint32_t group_num, uint32_t group_topk, uint32_t ef, uint32_t max_scan, float threshold,
                                 const uint64_t *exclude_bitset, uint32_t *out_groups, uint32_t *out_ngroups, uint64_t *out_keys,
                                 float *out_scores, uint32_t *out_counts) {
  ZRET(hnsw_group_args(h, queries, group_num, group_topk, ef, GroupOut{out_groups, out_ngroups, out_keys, out_scores, out_counts}));
  if (count == 0) return 0;
  zvec_hip_ctx_s *c = ctx ? ctx : h->defctx;
  std::lock_guard<std::mutex> g(c->mu);                // ONE critical section from the upload to the copy-out (zvec_hip_hnsw_search)
  ZCHK(hipSetDevice(h->device));
  GroupOut o{};
  {
    std::shared_lock<FairSharedMutex> r(h->rw);        // the row count the group numbers and the bitset are sized for
    if (!h->loaded) return ZVEC_HIP_ERR_NO_INDEX_LOADED;
    const uint64_t n = h->graph.n;
    if (n && !group_of_node) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
    ZRET(group_outputs(c, count, group_num, group_topk, &o));
    ZRET(c->grp_of.ensure(std::max<size_t>((size_t)n, 1) * 4));
    if (n) ZCHK(hipMemcpyAsync(c->grp_of.p, group_of_node, (size_t)n * 4, hipMemcpyHostToDevice, c->cur));
    ZRET(host_search_wrap_begin(c, queries, (size_t)count * h->row_bytes(), n ? exclude_bitset : nullptr, n, count, 1, c->cur));
    ZRET(hnsw_group_search_dev_locked(h, c, c->io_qp, count, c->grp_of.as<uint32_t>(), ngroups, group_num, group_topk, ef, max_scan,
                                      threshold, exclude_bitset && n ? c->io_ex.as<uint64_t>() : nullptr, o, c->cur));
  }
  return group_copy_out(c, o, count, group_num, group_topk, out_groups, out_ngroups, out_keys, out_scores, out_counts, c->cur);
}
