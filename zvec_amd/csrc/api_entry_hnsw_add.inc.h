// api_entry_hnsw_add.inc.h — C ABI entry points: appending rows to an HNSW graph on the device (zvec_hip_hnsw_add*, _reserve,
// _last_add_info; inside extern "C").  Stands behind HnswStreamer::add_impl / add_with_id_impl (hnsw_streamer.cc:426-585).  The rule
// is DESIGN §3c "Appending": the build's plan and apply step (hnsw_plan_call, hnsw_insert_apply, api_entry_hnsw_build.inc.h) started
// at s = the nodes already there, on arrays that grow (HnswGraph::resize, api_entry_hnsw.inc.h); host planning:
// host/hnsw_add_plan.h; device code: zvk_hnsw_build.hip.h.
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

// On a graph with nodes the plan is applied in place; on a handle without nodes (created, or after a load or a build of no rows) the
// call is a build of these rows that keeps what a reserve asked for: a fresh graph takes the old one's place on success.
static int hnsw_add_entry(zvec_hip_hnsw_t h, uint64_t count, const void *rows, bool rows_on_device, const uint64_t *keys,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  HnswWrite w(h);
  ZRET(w.open());
  const bool has = h->loaded && h->graph.n > 0;
  const HnswShape none;
  HnswInsertPlan pl;
  ZRET(hnsw_plan_call(has ? h->graph : none, h, true, count, rows, p, levels, pl));
  if (count == 0) return 0;                      // (nothing to insert, nothing changes)
  ZRET(w.quiesce());
  HnswGraph fresh;
  HnswGraph &g = has ? h->graph : fresh;
  HnswInsertDone done;
  ZRET(hnsw_insert_apply(h, g, pl, rows, rows_on_device, keys, done));
  hnsw_commit(h, g);
  if (!has) h->params = pl.q;
  h->added = true;
  h->adone = done;
  return 0;
}

// HnswStreamer::add_impl (hnsw_streamer.cc:426-503) for count rows: each ends in HnswAlgorithm::add_node(id, level, ctx)
int zvec_hip_hnsw_add(zvec_hip_hnsw_t h, uint64_t count, const void *rows, const uint64_t *keys, const zvec_hip_hnsw_build_params *p,
                      const uint32_t *levels) {
  return hnsw_add_entry(h, count, rows, false, keys, p, levels);
}

// the same behind a holder whose rows are in device memory already
int zvec_hip_hnsw_add_dev(zvec_hip_hnsw_t h, uint64_t count, const void *d_rows, const uint64_t *keys,
                          const zvec_hip_hnsw_build_params *p, const uint32_t *levels) {
  return hnsw_add_entry(h, count, d_rows, true, keys, p, levels);
}

// HnswStreamerEntity grows its storage chunk by chunk (hnsw_streamer_entity.cc); here the room is taken in one step
int zvec_hip_hnsw_reserve(zvec_hip_hnsw_t h, uint64_t rows, uint64_t upper_nodes) {
  if (!h) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (rows >= HNSW_PLAN_MAX_NODES || upper_nodes >= HNSW_PLAN_MAX_NODES) return ZVEC_HIP_ERR_OUT_OF_RANGE;
  HnswWrite w(h);
  ZRET(w.open());
  HnswGraph &g = h->graph;
  const bool has = h->loaded && g.n > 0;
  const uint32_t sf = h->params.scaling_factor ? h->params.scaling_factor : has && g.m ? g.m : 50;
  const uint64_t upper = upper_nodes ? upper_nodes : hnsw_reserve_upper(rows, sf);
  if (has && (rows > g.cap_rows || (g.stride && upper > g.cap_upper))) {
    ZRET(w.quiesce());
    HnswShape to = g;
    to.cap_rows = rows; to.cap_upper = upper;
    bool grew_rows, grew_upper;
    ZRET(g.resize(to, h->pad_bytes(), h->defctx->cur, grew_rows, grew_upper));
  }
  h->want_rows = std::max(h->want_rows, rows);
  h->want_upper = std::max(h->want_upper, upper);
  return 0;
}

// what the last add of `h` did
int zvec_hip_hnsw_last_add_info(zvec_hip_hnsw_t h, zvec_hip_hnsw_add_info *out) {
  if (!h || !out) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  std::shared_lock<FairSharedMutex> r(h->rw);
  if (!h->added) return ZVEC_HIP_ERR_NO_READY;
  const HnswInsertDone &d = h->adone;
  *out = zvec_hip_hnsw_add_info();
  hnsw_info_common(*out, d);
  out->first = d.first; out->count = d.count; out->rounds_one = d.one;
  out->grew_rows = d.grew_rows; out->grew_upper = d.grew_upper; out->restrided = d.restrided;
  out->cap_rows = d.cap_rows; out->cap_upper = d.cap_upper;
  return 0;
}
