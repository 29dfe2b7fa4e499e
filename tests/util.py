"""Shared helpers of the parity tests (compare a GPU result list with the oracle's)."""
import numpy as np


def tie_tolerant_compare(g_keys, g_scores, g_counts, o_keys, o_scores, o_counts, atol=0.0, rtol=0.0,
                         scale=None, what="", select_band=None):
    """Scores must agree rank by rank within atol + rtol*scale; key SETS must agree except where the
    disagreeing keys sit within the tolerance of the k-th (boundary) score — exact ties / near ties,
    which the reference itself resolves arbitrarily (heap.h:103-114,173-175).  With atol=rtol=0 this is
    bit-exact equality of scores and of ids outside exact boundary ties.
    `select_band` (per query, absolute): L2 lists are SELECTED with norm-expansion scores (error ~ ulp of the
    norms) and then re-scored directly (error ~ ulp of the distance); ids may differ from the oracle's only
    for candidates within that wider selection band of the k-th score, while the reported scores must
    agree within the tight atol/rtol."""
    nq = len(o_counts)
    assert len(g_counts) == nq
    for q in range(nq):
        c = int(o_counts[q])
        assert int(g_counts[q]) == c, "%s query %d: count %d vs oracle %d" % (what, q, g_counts[q], c)
        if c == 0:
            continue
        gs, os_ = g_scores[q, :c].astype(np.float64), o_scores[q, :c].astype(np.float64)
        sc = (np.abs(os_) if scale is None else np.full(c, float(scale if np.isscalar(scale) else scale[q])))
        tol = atol + rtol * sc
        band = 0.0 if select_band is None else float(select_band if np.isscalar(select_band) else select_band[q])
        if band == 0.0:
            assert np.all(np.abs(gs - os_) <= tol), "%s query %d: scores differ\n gpu %r\n ora %r" % (what, q, gs, os_)
        else:   # ranks may shift inside the band: compare the score multisets with band slack
            assert np.all(np.abs(gs - os_) <= tol + 2 * band), "%s query %d: scores differ\n gpu %r\n ora %r" % (what, q, gs, os_)
        assert np.all(np.diff(gs) >= 0), "%s query %d: gpu scores not ascending" % (what, q)
        gk, ok = set(g_keys[q, :c].tolist()), set(o_keys[q, :c].tolist())
        assert len(gk) == c, "%s query %d: duplicate keys in the gpu list" % (what, q)
        if band:
            om = {int(k_): s_ for k_, s_ in zip(o_keys[q, :c], os_)}
            for k_, s_ in zip(g_keys[q, :c], gs):
                if int(k_) in om:   # same document => the refined score must be tight
                    t_ = atol + rtol * (abs(om[int(k_)]) if scale is None else float(scale if np.isscalar(scale) else scale[q]))
                    assert abs(s_ - om[int(k_)]) <= t_, "%s query %d key %d: %r vs %r" % (what, q, k_, s_, om[int(k_)])
        if gk != ok:
            bound = os_[c - 1]
            btol = float(np.max(tol)) + band
            for k in gk - ok:
                s = gs[list(g_keys[q, :c]).index(k)]
                assert s >= bound - 2 * btol, "%s query %d: key %d (score %r) not in oracle list and not a boundary tie (%r)" % (what, q, k, s, bound)
            for k in ok - gk:
                s = os_[list(o_keys[q, :c]).index(k)]
                assert s >= gs[c - 1] - 2 * btol, "%s query %d: oracle key %d (score %r) missing from gpu list" % (what, q, k, s)


def exact_l2(base, queries):
    b = base.astype(np.float64)
    q = queries.astype(np.float64)
    return ((q[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def kmeans_lists(rng, base, nlist):
    """tiny host IVF structure for tests: random centroids = sampled rows, nearest assignment (fp64)."""
    n = base.shape[0]
    cent = base[rng.choice(n, nlist, replace=False)].astype(np.float32).copy()
    d = exact_l2(cent, base)            # [n][nlist]
    lab = d.argmin(1)
    order = np.argsort(lab, kind="stable")
    sizes = np.bincount(lab, minlength=nlist)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return cent, offs, order


def lpt_owner(sizes, nshards, tile=128):
    """the list -> shard map of zvec_hip_ivf_shard_map restated: lists by (tiles desc, id asc), each to the shard
    with the fewest 128-row tiles so far (lowest shard on ties).  SURVEY §8(e): whole lists, balanced by bytes."""
    sizes = np.asarray(sizes, np.int64)
    owner = np.zeros(sizes.size, np.uint32)
    if nshards <= 1:
        return owner
    load = [0] * nshards
    for l in np.argsort(-sizes, kind="stable"):
        g = min(range(nshards), key=lambda j: (load[j], j))
        owner[l] = g
        load[g] += (int(sizes[l]) + tile - 1) // tile
    return owner


# ---- search helpers of the half-width pre-selection tests (test_gpu_shadow.py, test_gpu_shadow_parity.py) -------------------------
def ivf_index(rng, base, nlist, metric="SquaredEuclidean", ratio=0.25, round_centroids=False):
    """an fp32 IVF searcher over `base` (kmeans_lists structure); returns it with what the oracle needs to search the same index"""
    import zvec_amd
    cent, offs, order = kmeans_lists(rng, base, nlist)
    if round_centroids:
        cent = np.round(cent)
    vecs, keys = base[order], order.astype(np.uint64)
    se = zvec_amd.HipIVFSearcher(base.shape[1], metric, scan_ratio=ratio, brute_force_threshold=10)
    assert se.load(cent, offs, vecs, keys) == 0
    return se, cent, offs, vecs, keys


def ivf_search(se, q, k, ctx=None, exclude=None, exclude_words=None):
    """host pointers: a search through the twin is certified inside the call"""
    ctx = ctx or se.create_context()
    ctx.set_topk(k)
    if exclude is not None:
        ctx.set_filter(exclude)
    if exclude_words is not None:
        ctx.set_exclude_bitset(exclude_words)
    assert se.search_impl(q, len(q), ctx) == 0
    return ctx.keys.copy(), ctx.scores.copy(), ctx.counts.copy()


def flat_search(se, q, k, exclude=None, exclude_words=None):
    return ivf_search(se, q, k, exclude=exclude, exclude_words=exclude_words)


def dev_lists(q, k, exclude_words):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    nq = len(q)
    keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    scores = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    counts = torch.zeros(nq, dtype=torch.int32, device="cuda")
    dex = None if exclude_words is None else torch.from_numpy(np.ascontiguousarray(exclude_words).view(np.int64)).cuda()
    return dq, keys, scores, counts, dex


def _host_lists(keys, scores, counts):
    return keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def ivf_search_dev(se, q, k, ctx=None, exclude_words=None):
    """device pointers: the search only enqueues, zvec_hip_ivf_shadow_certify finishes it; returns results + queries re-run"""
    import torch
    dq, keys, scores, counts, dex = dev_lists(q, k, exclude_words)
    nq = len(q)
    ctx = ctx or se.create_context()
    nprobe, max_scan = se.probe_params()
    ex = None if dex is None else dex.data_ptr()
    torch.cuda.synchronize()
    rc = se.search_dev(dq.data_ptr(), nq, k, nprobe, max_scan, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx, d_exclude=ex)
    assert rc == 0
    args = (dq.data_ptr(), nq, k, nprobe, max_scan, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx)
    rerun = se.shadow_certify(*args, d_exclude=ex)
    assert se.shadow_certify(*args, d_exclude=ex) == 0            # nothing pending any more
    torch.cuda.synchronize()
    return _host_lists(keys, scores, counts) + (rerun,)


def flat_search_dev(se, q, k, ctx=None, exclude_words=None):
    import torch
    dq, keys, scores, counts, dex = dev_lists(q, k, exclude_words)
    nq = len(q)
    ctx = ctx or se.create_context()
    ex = None if dex is None else dex.data_ptr()
    torch.cuda.synchronize()
    assert se.search_dev(dq.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx, d_exclude=ex) == 0
    args = (dq.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx)
    rerun = se.shadow_certify(*args, d_exclude=ex)
    assert se.shadow_certify(*args, d_exclude=ex) == 0
    torch.cuda.synchronize()
    return _host_lists(keys, scores, counts) + (rerun,)
