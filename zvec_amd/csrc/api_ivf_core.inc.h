// api_ivf_core.inc.h — IVF search on device pointers: coarse pass, plan, list scan, merge, large-k fallback
// Part of zvec_hip_api.hip (one translation unit; included in order, not standalone).

namespace {

// ---- IVF search core (device pointers) ------------------------------------------------------
// d_coarse_queries: the queries in the centroid store's own space when it has one (h->coarse_sep: an inner-product index whose
// centroid index the reference's builder trained in MIPS-converted space, ivf_builder.cc:552-555, searched through a MipsReformer,
// ivf_centroid_index.cc:273-297); nullptr otherwise
// The coarse pass may be taken apart from the rest (sharded IVF, SURVEY §8(e): every rank needs the same probe sets, and the
// pass — 2 x Q x nlist x d flop against replicated centroids — is the one piece of a rank's step that does not shrink with the
// number of ranks): `coarse` with out_idx set = run ONLY the coarse pass and leave the probe lists there ([count][nprobe] centroid
// ids in coarse-score order + [count] valid entries); with given_idx set = skip the coarse pass and plan from those lists.
struct CoarseSplit {
  const uint32_t *given_idx = nullptr, *given_cnt = nullptr;
  uint32_t *out_idx = nullptr, *out_cnt = nullptr;
};

int ivf_search_core(zvec_hip_ivf_s *h, zvec_hip_ctx_s *ctx, const void *d_queries, uint32_t count, uint32_t topk,
                    float threshold, uint32_t nprobe, uint32_t max_scan_count, int brute_force,
                    const uint64_t *d_exclude, const SearchOut &out, hipStream_t stream, const void *d_coarse_queries = nullptr,
                    const CoarseSplit &coarse = CoarseSplit(), ShadowMode mode = ShadowMode()) {
  const bool given = coarse.given_idx != nullptr, coarse_only = coarse.out_idx != nullptr;
  if ((given || coarse_only) && brute_force) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  if (h->coarse_sep && !brute_force && !given && d_coarse_queries == nullptr) return ZVEC_HIP_ERR_INVALID_ARGUMENT;
  const int cus = device_cus(ctx);
  const uint32_t nlist = h->lay.nlist;
  ctx->ivf_plan = IvfPlanMark();       // (zvec_hip_ctx_last_ivf_plan: set again where a route has enqueued all of its work)
  if (nprobe < 1) nprobe = 1;
  if (nprobe > nlist) nprobe = nlist;

  // A handful of queries (the product's count = 1 calls): both steps go wave-per-row instead of through the MFMA tile
  // kernels, whose few work items would each be a chain of dependent HBM round trips (1 query, 2M x 768, nprobe 32:
  // coarse 90 us + list scan 113 us for 6 + 96 MB).  Bound of the rows one query can scan: the nprobe largest lists.
  const uint64_t direct_rows = h->lay.rows_of_largest.size() > nprobe ? std::max<uint64_t>(1, h->lay.rows_of_largest[nprobe]) : ~0ull;
  // (measured, 2M x 768 fp32, nprobe 32 of 2048 lists, host-pointer calls: 1 query 223 -> 116 us, 2: 244 -> 153, 4: 290 -> 222,
  // 8: 390 -> 369, 16: 586 -> 655 — the direct route costs the same for every query, the tile route shares the lists)
  const bool direct = !brute_force && !coarse_only && count <= (uint32_t)knobs().ivf_direct_q && (uint64_t)count * direct_rows <= (4u << 20) &&
                      (double)count * (double)direct_rows * (double)h->lists.row_bytes() <= 2.5e9 &&
                      merge_fits(topk) && merge_fits(nprobe);

  // The direct route scores rows straight from the prepared query rows and needs no norms: when the caller's rows already ARE
  // prepared rows (no padding: dim_in == the scanned dims == whole 128-byte k-steps; 16-byte aligned) the preparation launch is
  // skipped — one kernel and one launch gap less in a chain of eight short dependent kernels (single query, 10M x 768:
  // 5 us + gap of the ~70 us one lane needs between two of its scoring kernels).
  const bool sep = h->coarse_sep && !brute_force && !given;      // (given probe lists: no coarse pass, only the lists' own space)
  const bool raw_rows = !sep && direct && h->lists.dim_in == h->lists.dscan && (size_t)h->lists.dpad * 4 == h->lists.row_bytes() &&
                        (reinterpret_cast<uintptr_t>(d_queries) & 15u) == 0 &&
                        !(ctx->pin_in.dev && d_queries == ctx->pin_in.dev);    // (rows in the host-mapped slot are read ONCE, by prep_queries)
  const float *qrows = raw_rows ? reinterpret_cast<const float *>(d_queries) : nullptr;
  if (!raw_rows) {
    // (a separate coarse space: the coarse pass runs on the coarse queries, then the list queries are prepared in their place)
    ZRET(prep_queries(ctx, sep ? h->cent : h->lists, sep ? d_coarse_queries : d_queries, count, FLT_MAX, stream));   // coarse pass: no RNN radius
    qrows = ctx->qpad.as<float>();
  }

  // the small-batch route: stream geometry and probe-rule arguments
  constexpr uint32_t RUN = 1024;                                        // one gather round of merge_kernel
  uint32_t stride = 0, runs = 0, *d_off = nullptr;
  bool block_topk = false;
  PlanArgs dp{};
  if (direct) {
    stride = (uint32_t)((direct_rows + 63) / 64 * 64);
    if (stride > RUN) stride = (stride + RUN - 1) / RUN * RUN;          // whole runs for the two-step selection
    runs = (stride + RUN - 1) / RUN;
    // long streams, ordinary k: the scoring blocks keep only the k best of their PKEYS_BLOCK candidates (pkeys_topk_kernel) and
    // ONE merge finishes; otherwise the whole score matrix is written and selected from in one or two steps
    block_topk = runs > 1 && topk <= PKEYS_TOPK_MAX;
    ZRET(ctx->plan.ensure(((size_t)3 * count + 8) * sizeof(uint32_t)));
    uint32_t *pb = ctx->plan.as<uint32_t>();
    dp.coarse_idx = ctx->coarse_idx.as<uint32_t>(); dp.coarse_cnt = ctx->coarse_cnt.as<uint32_t>();
    dp.nq = count; dp.nprobe = nprobe; dp.nlist = nlist; dp.max_scan_count = max_scan_count; dp.brute_force = 0;
    dp.list_size = h->tab.d_size.p; dp.list_size_global = h->tab.d_size_global.p;
    dp.q_nprobe = pb; dp.q_scanned = pb + count;
    d_off = pb + 2 * (size_t)count;
    if (ctx->profile && ctx->nprof < PROFILE_MAX && ctx->stats.p) {       // the slot prof_begin will take for this launch
      dp.work_stats = ctx->stats.as<unsigned long long>() + 2 * (size_t)ctx->nprof;     // (zero since the last profile reset)
    }
  }

  // 1. coarse assign: flat scan over the centroids, k = nprobe (IVFCentroidIndex::search)
  const uint32_t *probe_idx = coarse.given_idx, *probe_cnt = coarse.given_cnt;
  if (given) { dp.coarse_idx = probe_idx; dp.coarse_cnt = probe_cnt; }
  if (!brute_force && !given) {
    ZRET(ctx->coarse_keys.ensure((size_t)count * nprobe * sizeof(uint64_t)));
    ZRET(ctx->coarse_scores.ensure((size_t)count * nprobe * sizeof(float)));
    ZRET(ctx->coarse_idx.ensure((size_t)count * nprobe * sizeof(uint32_t)));
    ZRET(ctx->coarse_cnt.ensure((size_t)count * sizeof(uint32_t)));
    SearchOut co{ctx->coarse_keys.as<uint64_t>(), ctx->coarse_scores.as<float>(),
                 coarse_only ? coarse.out_idx : ctx->coarse_idx.as<uint32_t>(), coarse_only ? coarse.out_cnt : ctx->coarse_cnt.as<uint32_t>()};
    probe_idx = co.idx; probe_cnt = co.counts;
    if (direct) {
      const uint32_t cstride = (nlist + 63) / 64 * 64;
      const uint64_t cpairs = (uint64_t)count * cstride;
      ZRET(ctx->part_s.ensure(cpairs * 4));
      if (h->cent.f16)
        hipLaunchKernelGGL(rows_score_kernel<true>, dim3((unsigned)((cpairs + 3) / 4)), dim3(256), 0, stream, h->cent.base,
                           qrows, h->cent.dpad, h->cent.metric, nlist, count, cstride, ctx->part_s.as<float>());
      else
        hipLaunchKernelGGL(rows_score_kernel<false>, dim3((unsigned)((cpairs + 3) / 4)), dim3(256), 0, stream, h->cent.base,
                           qrows, h->cent.dpad, h->cent.metric, nlist, count, cstride, ctx->part_s.as<float>());
      dp.coarse_idx = co.idx; dp.coarse_cnt = co.counts;                  // (the buffers may just have grown)
      ZRET(launch_merge(merge_dense_rows(ctx->part_s.as<float>(), cstride, nprobe, FLT_MAX, nullptr, co), count, 256, stream));   // four waves share the row
    } else {
      ZRET(flat_scan_prepared(ctx, h->cent, count, nprobe, FLT_MAX, nullptr, co, stream, ScanRole::internal));
    }
    if (coarse_only) return 0;
  }
  if (sep) {
    ZRET(prep_queries(ctx, h->lists, d_queries, count, FLT_MAX, stream));      // from here on: the lists' own space
    qrows = ctx->qpad.as<float>();                                             // (the buffer may have grown: list rows wider than coarse rows)
  }
  if (direct) {
    // 2'. every query's probed rows as positions (same probe rule), 3'. one wave per (query, row): direct distance,
    // 4'. selection: the scoring blocks' own top-k lists -> the result, or (k > 64) two steps over the score matrix: runs of
    // 1024 candidates -> top-k lists -> the result (no refinement needed: the scores already are sum((q - b)^2))
    const uint64_t pairs = (uint64_t)count * stride;
    ZRET(ctx->direct_pos.ensure(pairs * 4));
    hipLaunchKernelGGL(ivf_expand_direct_kernel, dim3(nprobe, count), dim3(256), 0, stream, dp, h->tab.d_tile0.p, h->tab.d_dense0.p,
                       reinterpret_cast<const uint32_t *>(d_exclude), stride, d_off, ctx->direct_pos.as<uint32_t>());
    if (!block_topk) {
      ZRET(ctx->part_s.ensure(pairs * 4));
      ZRET(ctx->part_i.ensure(pairs * 4));
    }
    // NOT gated: handing the gate's event from one hardware queue to the other costs ~20 us, against a 50 us scoring kernel
    // (10M x 768, one query: two lanes 0.069 ms gated, 0.057 sharing the device freely).  (the radius is applied by the selection)
    const int pi = prof_begin(ctx, stream, (double)count * h->lists.dscan * h->lists.elem + (double)count * topk * 12.0, 0, 1);
    if (pi >= 0) ctx->prof_dscan[pi] = h->lists.dscan | (h->lists.f16 ? 0x80000000u : 0u);
    const uint32_t bpq = (stride + PKEYS_BLOCK - 1) / PKEYS_BLOCK;
    int lrc = 0;
    if (block_topk) {
      ZRET(ctx->direct_scores.ensure((uint64_t)count * bpq * topk * 4));
      ZRET(ctx->direct_idx.ensure((uint64_t)count * bpq * topk * 4));
      if (h->lists.f16)
        hipLaunchKernelGGL(pkeys_topk_kernel<true>, dim3(count * bpq), dim3(256), 0, stream, h->lists.base, qrows, h->lists.dpad,
                           h->metric, ctx->direct_pos.as<uint32_t>(), d_off, count, stride, topk, ctx->direct_scores.as<float>(),
                           ctx->direct_idx.as<uint32_t>());
      else
        hipLaunchKernelGGL(pkeys_topk_kernel<false>, dim3(count * bpq), dim3(256), 0, stream, h->lists.base, qrows, h->lists.dpad,
                           h->metric, ctx->direct_pos.as<uint32_t>(), d_off, count, stride, topk, ctx->direct_scores.as<float>(),
                           ctx->direct_idx.as<uint32_t>());
    } else {               // (the lists' metric is the index's: both are set once, by zvec_hip_ivf_create)
      lrc = launch_pkeys_score(h->lists, qrows, ctx->direct_pos.as<uint32_t>(), d_off, count, stride, ctx->part_s.as<float>(),
                               ctx->part_i.as<uint32_t>(), stream);
    }
    prof_end(ctx, stream, pi);
    ZRET(lrc);
    ZCHK(hipGetLastError());
    if (block_topk) {
      // (equal scores: list order, then entry order = the order of the candidate stream, as below)
      ZRET(launch_merge(merge_stream(ctx->direct_scores.as<float>(), ctx->direct_idx.as<uint32_t>(), bpq, topk, true, topk, threshold,
                                     h->lists.keys, out), count, 256, stream));
      ctx->q_nprobe = dp.q_nprobe; ctx->q_scanned = dp.q_scanned; ctx->last_count = count; ctx->last_list_count = nullptr;
      ctx->ivf_plan.route = ZVEC_HIP_IVF_ROUTE_DIRECT_BLOCK_TOPK; ctx->ivf_plan.nq = count; ctx->ivf_plan.nlist = nlist; ctx->ivf_plan.nprobe = nprobe;
      return 0;
    }
    // equal scores keep the reference's order — probe rank, then position in the list — which here is the ORDER of the
    // candidate stream, not the order of the positions
    const float *ps = ctx->part_s.as<float>();
    const uint32_t *ppos = ctx->part_i.as<uint32_t>();
    if (runs > 1) {
      // step 1: block (query, run) keeps the top-k of its 1024 candidates; step 2: a query's `runs` lists -> its result
      const uint64_t blocks = (uint64_t)count * runs;
      ZRET(ctx->direct_keys.ensure(blocks * topk * 8));
      ZRET(ctx->direct_scores.ensure(blocks * topk * 4));
      ZRET(ctx->direct_idx.ensure(blocks * topk * 4));
      ZRET(ctx->direct_cnt.ensure(blocks * 4));
      const SearchOut run{ctx->direct_keys.as<uint64_t>(), ctx->direct_scores.as<float>(), ctx->direct_idx.as<uint32_t>(),
                          ctx->direct_cnt.as<uint32_t>()};
      ZRET(launch_merge(merge_stream(ps, ppos, 1, RUN, true, topk, threshold, nullptr, run), (uint32_t)blocks, 64, stream));
      ZRET(launch_merge(merge_stream(run.scores, run.idx, runs, topk, true, topk, threshold, h->lists.keys, out), count, 256, stream));
    } else {
      ZRET(launch_merge(merge_stream(ps, ppos, 1, stride, true, topk, threshold, h->lists.keys, out), count, 64, stream));
    }
    ctx->q_nprobe = dp.q_nprobe; ctx->q_scanned = dp.q_scanned; ctx->last_count = count; ctx->last_list_count = nullptr;
    ctx->ivf_plan.route = ZVEC_HIP_IVF_ROUTE_DIRECT_SELECT; ctx->ivf_plan.nq = count; ctx->ivf_plan.nlist = nlist; ctx->ivf_plan.nprobe = nprobe;
    return 0;
  }

  // 2. plan: list-major work items
  // list scan shape: 16x16x4 MFMA tiles, 32 query rows per work item as two 16-row halves (the second is
  // skipped when the item has <= 16 rows); a list probed by more than 32 queries is dealt as several items
  const int ng = 0;
  if (scan_lds_bytes(1, topk, true) > LDS_LIMIT - 1024) {
    // Large k (beyond ~470): the result lists no longer fit beside the staging buffers.  Rare, so served by the plain
    // route: expand every query's probed lists into positions, score each (query, row) pair directly, select.
    if (!merge_fits(topk)) return ZVEC_HIP_ERR_UNSUPPORTED;
    PlanArgs p{};
    p.coarse_idx = probe_idx; p.coarse_cnt = probe_cnt;
    p.nq = count; p.nprobe = nprobe; p.nlist = nlist; p.max_scan_count = max_scan_count; p.brute_force = brute_force;
    p.list_size = h->tab.d_size.p; p.list_size_global = h->tab.d_size_global.p;
    ZRET(ctx->plan.ensure(((size_t)2 * count + 8) * sizeof(uint32_t)));
    uint32_t *d_rows = ctx->plan.as<uint32_t>(), *d_off = d_rows + count;
    // upper bound of the rows one query scans here: the np largest local lists
    uint64_t maxlen = 0;
    {
      std::vector<uint32_t> sz(h->lay.size);
      const uint32_t np = brute_force ? nlist : nprobe;
      std::partial_sort(sz.begin(), sz.begin() + np, sz.end(), std::greater<uint32_t>());
      for (uint32_t i = 0; i < np; ++i) maxlen += sz[i];
    }
    if (maxlen == 0) maxlen = 1;
    if ((uint64_t)count * maxlen >= 0xffffffffull) return ZVEC_HIP_ERR_OUT_OF_RANGE;   // (slice the batch)
    hipLaunchKernelGGL(ivf_expand_kernel<false>, dim3((count + 3) / 4), dim3(256), 0, stream, p, h->tab.d_tile0.p, h->tab.d_dense0.p,
                       nullptr, d_rows, nullptr, nullptr);
    hipLaunchKernelGGL(u32_exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, d_rows, d_off, count, d_off + count);
    ZCHK(hipGetLastError());
    uint32_t total_rows = 0;
    ZCHK(hipMemcpyAsync(&total_rows, d_off + count, 4, hipMemcpyDeviceToHost, stream));
    ZCHK(hipStreamSynchronize(stream));
    Scoped<uint32_t> d_pos;
    ZRET(d_pos.alloc(std::max<uint32_t>(total_rows, 1)));
    hipLaunchKernelGGL(ivf_expand_kernel<true>, dim3((count + 3) / 4), dim3(256), 0, stream, p, h->tab.d_tile0.p, h->tab.d_dense0.p,
                       reinterpret_cast<const uint32_t *>(d_exclude), nullptr, d_off, d_pos);
    ZCHK(hipGetLastError());
    const uint64_t pairs = (uint64_t)count * maxlen;
    ZRET(ctx->part_s.ensure(pairs * 4));
    ZRET(ctx->part_i.ensure(pairs * 4));
    // (re-prepare the queries with the caller's RNN radius: the coarse pass ran without one)
    ZRET(prep_queries(ctx, h->lists, d_queries, count, threshold, stream));
    ZRET(launch_pkeys_score(h->lists, ctx->qpad.as<float>(), d_pos, d_off, count, (uint32_t)maxlen, ctx->part_s.as<float>(),
                            ctx->part_i.as<uint32_t>(), stream));
    ZRET(launch_merge(merge_stream(ctx->part_s.as<float>(), ctx->part_i.as<uint32_t>(), 1, (uint32_t)maxlen, false, topk, threshold,
                                   h->lists.keys, out), count, 64, stream));
    ZCHK(hipStreamSynchronize(stream));    // d_pos is freed on return
    ctx->q_nprobe = nullptr; ctx->q_scanned = nullptr; ctx->last_count = 0;
    ctx->ivf_plan.route = ZVEC_HIP_IVF_ROUTE_LARGE_K; ctx->ivf_plan.nq = count; ctx->ivf_plan.nlist = nlist;
    ctx->ivf_plan.nprobe = brute_force ? nlist : nprobe; ctx->ivf_plan.brute_force = brute_force ? 1u : 0u;
    return 0;
  }
  // Half-width pre-selection (zvk_shadow.hip.h): the scan reads the fp16 twin of the lists and keeps k' > k rows per query, which
  // are re-scored on the fp32 rows and certified below.  Not with an RNN radius (it would have to be widened by the rounding bound),
  // not for search_bf, not on the certify step's own re-run.
  ShadowTwin &tw = h->shadow;
  uint32_t kp = 0;
  if (tw.on && tw.st.base && mode.kind != ShadowMode::fp32_only && !brute_force && !(threshold < FLT_MAX) && topk <= 32 && tw.gov.allow()) {
    kp = tw.pick_kp(mode.kp, topk);
    if (kp <= topk || scan_lds_bytes(1, kp, true) > LDS_LIMIT - 1024) kp = 0;
  }
  const bool use_shadow = kp != 0;
  const uint32_t ks = use_shadow ? kp : topk;                            // k of the list scan and of its merge
  ctx->sh.count = 0;
  const uint32_t rows_per_group = 32;
  const uint64_t npairs = (uint64_t)count * (brute_force ? nlist : nprobe);
  // layout of the plan buffer (u32 words)
  size_t off = 0;
  auto take = [&](size_t words) { size_t o = off; off += (words + 3) & ~(size_t)3; return o; };
  size_t o_qnprobe = take(count), o_qscanned = take(count), o_qnslots = take(count), o_slotbegin = take(count + 1);
  size_t o_lcount = take(nlist), o_lfill = take(nlist), o_lqoff = take(nlist + 1), o_itemoff = take(nlist + 1);
  size_t o_queue = take(4);
  size_t o_ltpc = take(nlist);
  size_t o_total = take(4), o_csrq = take(npairs), o_csrslot = take(npairs);
  ZRET(ctx->plan.ensure(off * sizeof(uint32_t)));
  uint32_t *pb = ctx->plan.as<uint32_t>();
  // list_count + list_fill and the work-queue head zeroed, shared bounds reset (the coarse pass may have left
  // centroid-score bounds behind): one launch
  // chunk length of this search: the lists it can touch (at most count x nprobe of them) should give a few items per
  // resident work-group — a single query probing 40 lists needs one-tile items to use the chip at all, a batch of
  // 1024 the index-wide default
  uint32_t tpc = h->lay.tiles_per_chunk;
  {
    const uint64_t lists_touched = std::min<uint64_t>(nlist, (uint64_t)count * (brute_force ? nlist : nprobe));
    const uint64_t est_tiles = std::max<uint64_t>(1, h->lay.local_tiles * lists_touched / std::max<uint32_t>(nlist, 1));
    const uint64_t t = est_tiles / (4ull * (uint64_t)device_cus(ctx) * 3ull);
    // never one-tile items: they double the slots the merge has to fold for nothing (measured, 10M x 768, nprobe 38:
    // batch 1 best at 2 tiles, batch 8 at 4, batch 32 at 4-8, batch 1024 at the index default)
    const uint64_t lo = est_tiles >= 4096 ? 4 : 2;
    tpc = (uint32_t)std::min<uint64_t>(h->lay.tiles_per_chunk, std::max<uint64_t>(lo, t));
    if (knobs().ivf_tpc) tpc = (uint32_t)knobs().ivf_tpc;
  }
  {
    ZRET(ctx->gtau.ensure((size_t)count * sizeof(uint32_t)));
    const uint32_t nzero = (uint32_t)(o_lqoff - o_lcount);
    const uint32_t nthr = std::max<uint32_t>(std::max<uint32_t>(nzero, count), std::max<uint32_t>(nlist, 4));
    hipLaunchKernelGGL(ivf_reset_kernel, dim3((nthr + 255) / 256), dim3(256), 0, stream, pb + o_lcount, nzero, pb + o_queue,
                       ctx->gtau.as<uint32_t>(), count, threshold, pb + o_ltpc, h->tab.d_tail.p, nlist, tpc);
    ZCHK(hipGetLastError());
  }
  PlanArgs p{};
  p.coarse_idx = probe_idx; p.coarse_cnt = probe_cnt;
  p.nq = count; p.nprobe = nprobe; p.nlist = nlist; p.max_scan_count = max_scan_count; p.brute_force = brute_force;
  p.list_size = h->tab.d_size.p; p.list_size_global = h->tab.d_size_global.p; p.list_order = h->tab.d_order.p;
  p.list_tpc = pb + o_ltpc;
  p.rows_per_group = rows_per_group;
  p.q_nprobe = pb + o_qnprobe; p.q_scanned = pb + o_qscanned; p.q_nslots = pb + o_qnslots; p.slot_begin = pb + o_slotbegin;
  p.list_count = pb + o_lcount; p.list_fill = pb + o_lfill; p.list_qoff = pb + o_lqoff; p.item_off = pb + o_itemoff;
  p.total_items = pb + o_total; p.csr_q = pb + o_csrq; p.csr_slot = pb + o_csrslot;
  ctx->q_nprobe = p.q_nprobe; ctx->q_scanned = p.q_scanned; ctx->last_count = count;
  ctx->last_list_count = p.list_count;
  if (ctx->profile && ctx->nprof < PROFILE_MAX && ctx->stats.p)      // the slot prof_begin will take for this launch
    p.work_stats = ctx->stats.as<unsigned long long>() + 2 * (size_t)ctx->nprof;
  hipLaunchKernelGGL(plan_wave_kernel<false>, dim3((count + 3) / 4), dim3(256), 0, stream, p);
  // (a pipelined context — one of several lanes, i.e. gated or driven on a caller's stream — runs beside another lane's
  // resident list scan: a 1024-thread work-group is not dispatched until that scan drains — 714 us for this 20 us kernel
  // in the round-2 trace — four waves are)
  const bool pipelined = ctx->gate != nullptr || stream != ctx->own;
  const uint32_t scan_threads = pipelined ? 256 : 1024;
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(scan_threads), 0, stream, p);
  hipLaunchKernelGGL(plan_wave_kernel<true>, dim3((count + 3) / 4), dim3(256), 0, stream, p);
  ZCHK(hipGetLastError());

  // 3. scan.  Upper bound of slots: every probed list contributes its chunks; the worst case is a query that
  //    probes the nprobe lists with the most chunks.
  const std::vector<uint32_t> &sz = h->lay.size;
  uint64_t slots_bound;
  {
    std::vector<uint32_t> chunks(nlist);
    for (uint32_t l = 0; l < nlist; ++l)
    {
      const uint32_t t = level_tpc(h->lay.tail[l], tpc);
      chunks[l] = sz[l] ? (uint32_t)((ivf_tiles(sz[l]) + t - 1) / t) : 0;
    }
    uint32_t np = brute_force ? nlist : nprobe;
    std::partial_sort(chunks.begin(), chunks.begin() + np, chunks.end(), std::greater<uint32_t>());
    uint64_t s = 0;
    for (uint32_t i = 0; i < np; ++i) s += chunks[i];
    slots_bound = s * count;
  }
  if (slots_bound == 0) slots_bound = 1;
  ZRET(ctx->part_s.ensure(slots_bound * ks * sizeof(float)));
  ZRET(ctx->part_i.ensure(slots_bound * ks * sizeof(uint32_t)));

  const StoreView &sst = use_shadow ? tw.st : h->lists;                      // the store the list scan streams
  ScanArgs a = scan_operands(ctx, sst, d_exclude, threshold);     // (the twin's metric is the lists', which is the index's)
  if (use_shadow) {
    ZRET(shadow_prep_queries(ctx, sst, d_queries, count, stream));
    a.queries = ctx->sh.q16.as<float>(); a.qnorm = ctx->sh.qn16.as<float>();
  }
  a.k = ks; a.mode = 1; a.nq = count; a.n = h->lists.n; a.ndense = h->lay.count_local; a.tiles_per_chunk = tpc; a.list_tpc = pb + o_ltpc;
  a.total_items = p.total_items; a.queue = pb + o_queue; a.list_order = h->tab.d_order.p; a.item_off = p.item_off; a.list_tile0 = h->tab.d_tile0.p; a.list_size = h->tab.d_size.p;
  a.list_dense0 = h->tab.d_dense0.p; a.list_qoff = p.list_qoff; a.csr_q = p.csr_q; a.csr_slot = p.csr_slot; a.nlist = nlist;
  a.part_s = ctx->part_s.as<float>(); a.part_i = ctx->part_i.as<uint32_t>();
  // algorithmic bytes of the list scan = rows of the DISTINCT probed lists (counted on device from
  // the plan: plan_scan_kernel's work_stats) + the query rows + the result lists
  gate_enter(ctx, stream);
  int pi = prof_begin(ctx, stream, (double)count * sst.dscan * sst.elem + (double)count * ks * 12.0, 0, 1);
  if (pi >= 0) ctx->prof_dscan[pi] = sst.dscan | (sst.f16 ? 0x80000000u : 0u);
  const int lrc = launch_scan_ng(ng, a, sst.f16, 0x7fffffffu, cus, stream);
  prof_end(ctx, stream, pi);
  gate_leave(ctx, stream);
  ZRET(lrc);
  {
    // the plan is complete on the stream from here on: remember where its arrays lie (host words only, nothing enqueued)
    IvfPlanMark &m = ctx->ivf_plan;
    m.route = ZVEC_HIP_IVF_ROUTE_TILE; m.scan_threads = scan_threads; m.nq = count; m.nlist = nlist;
    m.nprobe = brute_force ? nlist : nprobe; m.tpc = tpc; m.rows_per_group = rows_per_group; m.brute_force = brute_force ? 1u : 0u;
    m.slots_bound = slots_bound; m.npairs = npairs; m.words = off;
    m.o_qnprobe = o_qnprobe; m.o_qscanned = o_qscanned; m.o_qnslots = o_qnslots; m.o_slotbegin = o_slotbegin; m.o_lcount = o_lcount;
    m.o_lqoff = o_lqoff; m.o_itemoff = o_itemoff; m.o_ltpc = o_ltpc; m.o_total = o_total; m.o_csrq = o_csrq; m.o_csrslot = o_csrslot;
  }

  // 4. merge the per-(query, probe, chunk) partial lists in probe order
  if (use_shadow) {
    // the k' pre-selected rows of every query in shadow-score order -> their true scores -> the k best + the certificate
    SearchOut pre;
    ZRET(shadow_lists(ctx, count, kp, &pre));
    ZRET(launch_merge(merge_slot_ranges(a.part_s, a.part_i, p.slot_begin, kp, a.gtau, kp, threshold, h->lists.keys, pre), count,
                      merge_threads(count), stream));
    return shadow_rescore_select(ctx, h->lists, tw, count, kp, topk, out, stream);
  }
  uint32_t *ridx = out.idx;
  if (h->metric == ZVEC_HIP_METRIC_L2 && ridx == nullptr) {
    ZRET(ctx->ridx.ensure((size_t)count * topk * sizeof(uint32_t)));
    ridx = ctx->ridx.as<uint32_t>();
  }
  ZRET(launch_merge(merge_slot_ranges(a.part_s, a.part_i, p.slot_begin, topk, a.gtau, topk, threshold, h->lists.keys,
                                      SearchOut{out.keys, out.scores, ridx, out.counts}), count, merge_threads(count), stream));
  ZRET(refine_l2(ctx, h->lists, count, topk, threshold, out.keys, out.scores, ridx, out.counts, stream));
  return 0;
}

constexpr size_t PIN_LIMIT = 256u << 10;  // staging through pinned memory up to 256 KiB per direction (above that the extra
                                          // host copy costs more than the pageable transfer: batch 1024 lost 2 %)

// wait policy 1: the last thing on the stream writes the call's epoch into a pinned word the host polls
__global__ void done_word_kernel(volatile uint32_t *word, uint32_t epoch) {
  __threadfence_system();
  *word = epoch;
}

// A host-pointer call waits for its stream here (RuntimeOpts::wait).  Everything the call enqueued is on `stream`.
int host_wait(zvec_hip_ctx_s *ctx, hipStream_t stream) {
  const int policy = ropts().wait.load(std::memory_order_relaxed);
  if (policy == 1 && ctx->done_word.ensure(64) == 0 && ctx->done_word.dev) {
    // a plain word in pinned memory: no runtime call (and none of its locks) per poll; a short spin for the single caller's
    // latency, then the CPU is handed on between polls — with more callers than CPUs the waiting threads no longer hold the
    // time slices the launching ones need
    volatile uint32_t *w = static_cast<volatile uint32_t *>(ctx->done_word.p);
    const uint32_t epoch = ++ctx->done_epoch ? ctx->done_epoch : ++ctx->done_epoch;      // (0 = the word's initial value)
    hipLaunchKernelGGL(done_word_kernel, dim3(1), dim3(1), 0, stream, static_cast<volatile uint32_t *>(ctx->done_word.dev), epoch);
    ZCHK(hipGetLastError());
    // Spin while the answer is close, sleep while it is not.  A lone caller's search ends ~0.1 ms after its last launch: it is
    // found by the spin.  With many callers sharing the GPU a call waits a millisecond or more; a thread that spun (or
    // sched_yield-ed on a core of its own) through that would burn a whole CPU — 64 such callers exhaust a 16-CPU quota in a
    // quarter of every scheduler period and are then all frozen for the rest of it (measured: p99 78 ms, throughput / 3).  So a
    // context whose previous wait was long goes to sleep at once, in steps that follow the time it has already waited.
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed = [&]() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); };
    const uint64_t est = ctx->last_wait_ns;                 // how long this context's waits have been taking
    if (est > 300000) {
      // sleeping mode.  HALF the expected wait in one sleep, the rest in steps of 1/32 of it: the completion is then noticed within
      // ~3 % (+ the timer slack) and MEASURED (it falls into the polled half), so the estimate follows the truth both ways.  A
      // sleep that wakes to a finished call has only learnt "at most this long": the estimate is halved — it must never feed on
      // its own oversleeping (an estimate of 60 ms once, from a first call that allocated its workspace, would otherwise hold
      // every later 5 ms call for 45 ms).
      const uint64_t first = std::min<uint64_t>(est / 2, 20000000);
      struct timespec ts = {0, (long)first};
      nanosleep(&ts, nullptr);
      if (*w == epoch) { ctx->last_wait_ns = first; return 0; }
      const uint64_t step = std::min<uint64_t>(200000, std::max<uint64_t>(20000, est / 32));
      for (uint32_t it = 0;; ++it) {
        struct timespec t2 = {0, (long)step};
        nanosleep(&t2, nullptr);
        if (*w == epoch) { ctx->last_wait_ns = elapsed(); return 0; }
        if ((it & 63) == 63) {
          // a fault on the stream would leave the word unwritten for ever: ask the runtime now and then
          hipError_t q = hipStreamQuery(stream);
          if (q != hipSuccess && q != hipErrorNotReady) { ZCHK(q); }
          if (q == hipSuccess && *w != epoch && elapsed() > 5000000000ull) break;
        }
      }
    } else {
      // spinning mode: the answer is ~0.1 ms away
      for (uint32_t it = 0;; ++it) {
        if (*w == epoch) { ctx->last_wait_ns = elapsed(); return 0; }
        __builtin_ia32_pause();
        if ((it & 63) == 63 && elapsed() > 400000) { ctx->last_wait_ns = 600000; break; }     // longer than a lone call: sleep from now on
      }
      for (uint32_t it = 0;; ++it) {
        struct timespec t2 = {0, 50000};
        nanosleep(&t2, nullptr);
        if (*w == epoch) { ctx->last_wait_ns = elapsed(); return 0; }
        if ((it & 63) == 63) {
          hipError_t q = hipStreamQuery(stream);
          if (q != hipSuccess && q != hipErrorNotReady) { ZCHK(q); }
          if (q == hipSuccess && *w != epoch && elapsed() > 5000000000ull) break;
        }
      }
    }
    ZCHK(hipStreamSynchronize(stream));
    return 0;
  }
  if (policy == 2) {
    if (!ctx->block_ev) ZCHK(hipEventCreateWithFlags(&ctx->block_ev, hipEventBlockingSync | hipEventDisableTiming));
    ZCHK(hipEventRecord(ctx->block_ev, stream));
    ZCHK(hipEventSynchronize(ctx->block_ev));
    return 0;
  }
  ZCHK(hipStreamSynchronize(stream));
  return 0;
}

// Host-pointer entry points: queries (and an exclude set) in, keys | scores | counts out.  Small transfers skip the copy engine
// (RuntimeOpts::zerocopy): the rows are put into the context's pinned slot, which is mapped into the device's address space,
// and the first kernel of the search — prep_queries — reads them over the host link in place (ctx->io_qp); the result arrays
// are views into the mapped result slot, so the last kernels of the chain (merge / re-score / re-sort) write the answer straight
// into host memory and the call ends with ONE wait and three memcpys.  A copy command costs more than the 3 KB it moves: the
// copy engine's own dispatch and its hand-over to the compute queue and back (single query, 10M x 768: 0.109 -> see DESIGN §3).
int host_search_wrap_begin(zvec_hip_ctx_s *ctx, const void *queries, size_t qbytes, const uint64_t *exclude,
                           uint64_t nbits, uint32_t count, uint32_t topk, hipStream_t stream) {
  const int zc = ropts().zerocopy.load(std::memory_order_relaxed);      // bit 0: queries read in place, bit 1: results written in place
  ZRET(ctx->io_q.ensure(qbytes));
  ctx->io_qp = ctx->io_q.p;
  if (qbytes <= PIN_LIMIT && ctx->pin_in.ensure(qbytes) == 0) {
    memcpy(ctx->pin_in.p, queries, qbytes);              // (the previous call's transfer has been waited for)
    if ((zc & 1) && ctx->pin_in.dev)
      ctx->io_qp = ctx->pin_in.dev;
    else
      ZCHK(hipMemcpyAsync(ctx->io_q.p, ctx->pin_in.p, qbytes, hipMemcpyHostToDevice, stream));
  } else {
    ZCHK(hipMemcpyAsync(ctx->io_q.p, queries, qbytes, hipMemcpyHostToDevice, stream));
  }
  if (exclude) {
    size_t words = (size_t)((nbits + 63) / 64);
    ZRET(ctx->io_ex.ensure(words * 8 + 8));
    ZCHK(hipMemcpyAsync(ctx->io_ex.p, exclude, words * 8, hipMemcpyHostToDevice, stream));
  }
  // keys | scores | counts in ONE buffer (16-byte aligned parts): a single copy brings a result back — or none at all
  const size_t kb = (size_t)count * topk * sizeof(uint64_t), sb = ((size_t)count * topk * sizeof(float) + 15) & ~(size_t)15,
               cb = (size_t)count * sizeof(uint32_t);
  char *o = nullptr;
  ctx->out_mapped = false;
  if ((zc & 2) && kb + sb + cb <= PIN_LIMIT && ctx->pin_out.ensure(kb + sb + cb) == 0 && ctx->pin_out.dev) {
    o = static_cast<char *>(ctx->pin_out.dev);
    ctx->out_mapped = true;
  } else {
    ZRET(ctx->io_out.ensure(kb + sb + cb));
    o = ctx->io_out.as<char>();
  }
  ctx->io_keys.p = o;
  ctx->io_scores.p = o + kb;
  ctx->io_counts.p = o + kb + sb;
  return 0;
}

int host_search_wrap_end(zvec_hip_ctx_s *ctx, uint32_t count, uint32_t topk, uint64_t *out_keys, float *out_scores,
                         uint32_t *out_counts, hipStream_t stream) {
  const size_t kb = (size_t)count * topk * sizeof(uint64_t), sbytes = (size_t)count * topk * sizeof(float),
               sb = (sbytes + 15) & ~(size_t)15, cb = (size_t)count * sizeof(uint32_t);
  if (ctx->out_mapped) {
    ZRET(host_wait(ctx, stream));
    const char *h = static_cast<const char *>(ctx->pin_out.p);
    memcpy(out_keys, h, kb);
    memcpy(out_scores, h + kb, sbytes);
    memcpy(out_counts, h + kb + sb, cb);
    return 0;
  }
  if (kb + sb + cb <= PIN_LIMIT && ctx->pin_out.ensure(kb + sb + cb) == 0) {
    char *h = static_cast<char *>(ctx->pin_out.p);
    ZCHK(hipMemcpyAsync(h, ctx->io_out.p, kb + sb + cb, hipMemcpyDeviceToHost, stream));
    ZRET(host_wait(ctx, stream));
    memcpy(out_keys, h, kb);
    memcpy(out_scores, h + kb, sbytes);
    memcpy(out_counts, h + kb + sb, cb);
    return 0;
  }
  ZCHK(hipMemcpyAsync(out_keys, ctx->io_keys.p, kb, hipMemcpyDeviceToHost, stream));
  ZCHK(hipMemcpyAsync(out_scores, ctx->io_scores.p, sbytes, hipMemcpyDeviceToHost, stream));
  ZCHK(hipMemcpyAsync(out_counts, ctx->io_counts.p, cb, hipMemcpyDeviceToHost, stream));
  ZRET(host_wait(ctx, stream));
  return 0;
}

}  // namespace
