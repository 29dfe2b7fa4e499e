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


# ---- labelling reference of the IVF build tests (test_gpu_label_parity.py, test_gpu_build.py, test_label_reference_cpu.py) -------
_METRIC_IDS = {"SquaredEuclidean": 0, "InnerProduct": 1, "Cosine": 2, 0: 0, 1: 1, 2: 2}


def label_scan_width(dim, dtype, metric="SquaredEuclidean"):
    """(scanned dims, padded scan width) of a centroid store: cosine rows end with their norm (one float, or two half slots),
    which is not scanned; the scan is padded to the k-step, 32 floats or 64 halves (StoreView::configure)."""
    half = np.dtype(dtype) == np.float16
    dscan = dim - ((2 if half else 1) if _METRIC_IDS[metric] == 2 else 0)
    step = 64 if half else 32
    return dscan, (dscan + step - 1) // step * step


def label_reference(cent, rows, metric="SquaredEuclidean", ignore=(), chunk=None):
    """Nearest-centroid labelling in plain fp64, with the error bound a correct fp32 kernel may use up.

    Returns (s64 [n][nlist], arg [n], gap [n], E [n][nlist]):
      s64   L2: sum((x - c)^2) summed directly; InnerProduct: -x.c; Cosine: 1 - x.c over the scanned dims
      arg   fp64 arg-min, the FIRST minimum on ties (numpy's argmin)
      gap   runner-up score minus the minimum, per row (+inf with one centroid)
      E     per-pair bound on |kernel score - s64|
    Centroid ids in `ignore` are left out of arg / gap (their score counts as +inf): a centroid copied to a LATER id sees the same
    arithmetic as the original and must never be returned, so it is no competitor.

    The bound is derived, not tuned.  The kernels multiply exactly (fp32 operands through v_mfma_f32_32x32x2f32; a product of two
    halves has 22 significant bits) and accumulate in fp32 in SOME order, so with u = 2^-24 a length-d sum of terms t_i is off by
    at most gamma_d * sum|t_i|, gamma_d ~ d u.  For gamma the project's own accumulation slack is taken, (d + 8) 2^-23 with d the
    PADDED scan width (zvk_shadow.hip.h: twice the textbook bound, because the order inside the matrix cores is not documented).
      InnerProduct  score = -dot: one sum of d exact products, the final fused multiply-add by -1 is exact
                      E = gamma * sum|x_i||c_i|
      L2            score = fma(-2, dot, |x|^2 + |c|^2): the two norms are fp32 sums of d squares (gamma |x|^2, gamma |c|^2), the
                    dot carries 2 gamma sum|x_i c_i|, the addition of the norms and the fma one rounding each, of values no larger
                    than (|x| + |c|)^2.  With sum|x_i c_i| <= |x||c| all of it is inside
                      E = gamma * (|x| + |c|)^2       (the "+ 8" of gamma pays for the two roundings)
                    The 256-tile kernel compares |c|^2 - 2 x.c, which drops |x|^2 and its error: the same E covers it.  A score
                    clamped at 0 moved towards the true (non-negative) value.
      Cosine        score = fma(-1, dot, 1): the inner-product bound plus one rounding of a value of at most 1 + sum|x_i c_i|
                      E = gamma * sum|x_i||c_i| + 2^-24 (1 + sum|x_i||c_i|)
    Acceptance (label_accept): label g of row x is right iff s64(x, g) - min_j s64(x, j) <= E(x, g) + E(x, argmin): the kernel
    saw g no worse than the arg-min, each off by its own bound at most.  A row is AMBIGUOUS when its gap is within E(x, argmin)
    + E(x, runner-up); only such rows may be labelled differently from arg."""
    m = _METRIC_IDS[metric]
    c64 = np.asarray(cent).astype(np.float64)
    x64 = np.asarray(rows).astype(np.float64)
    dscan, dpad = label_scan_width(c64.shape[1], np.asarray(cent).dtype, m)
    c64, x64 = c64[:, :dscan], x64[:, :dscan]
    n, nlist = x64.shape[0], c64.shape[0]
    gamma = (dpad + 8) * 2.0 ** -23
    s64 = np.empty((n, nlist))
    E = np.empty((n, nlist))
    cn = np.sqrt((c64 ** 2).sum(1))
    ca = np.abs(c64)
    step = chunk or max(1, (1 << 22) // max(1, nlist * dscan))
    for o in range(0, n, step):
        x = x64[o:o + step]
        if m == 0:
            d = x[:, None, :] - c64[None]
            s64[o:o + step] = np.einsum("ijk,ijk->ij", d, d)
            E[o:o + step] = gamma * (np.sqrt((x ** 2).sum(1))[:, None] + cn[None]) ** 2
        else:
            dot = np.einsum("ik,jk->ij", x, c64)
            mag = np.einsum("ik,jk->ij", np.abs(x), ca)
            s64[o:o + step] = -dot if m == 1 else 1.0 - dot
            E[o:o + step] = gamma * mag + (2.0 ** -24 * (1.0 + mag) if m == 2 else 0.0)
    comp = s64.copy()
    if len(ignore):
        comp[:, list(ignore)] = np.inf
    arg = comp.argmin(1)
    if nlist - len(ignore) > 1:
        two = np.partition(comp, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(n, np.inf)
    return s64, arg, gap, E


def label_runner_up(s64, arg, ignore=()):
    comp = s64.copy()
    if len(ignore):
        comp[:, list(ignore)] = np.inf
    comp[np.arange(len(arg)), arg] = np.inf
    return comp.argmin(1)


def label_ambiguous(s64, arg, gap, E, ignore=()):
    """rows whose fp64 runner-up gap is within the two bounds: the only rows a correct kernel may label differently from arg"""
    if s64.shape[1] - len(ignore) < 2:
        return np.zeros(len(arg), bool)
    i = np.arange(len(arg))
    return gap <= E[i, arg] + E[i, label_runner_up(s64, arg, ignore)]


def label_accept(s64, arg, E, labels):
    """the acceptance rule, per row; a label outside [0, nlist) is never accepted"""
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab < s64.shape[1])
    g = np.where(ok, lab, 0)
    i = np.arange(len(arg))
    return ok & (s64[i, g] - s64[i, arg] <= E[i, g] + E[i, arg])


def check_labels(cent, rows, metric, labels, ignore=(), cap=0.01, what="", ref=None):
    """every label accepted, none of them an ignored (duplicate) id, no more differences from the fp64 arg-min than there are
    ambiguous rows, and (cap not None) at most `cap` of the rows ambiguous — a condition on the inputs.  Returns the reference."""
    ref = ref or label_reference(cent, rows, metric, ignore)
    s64, arg, gap, E = ref
    lab = np.asarray(labels).astype(np.int64)
    acc = label_accept(s64, arg, E, lab)
    bad = np.nonzero(~acc)[0]
    assert bad.size == 0, "%s: %d labels outside the band, first rows %r got %r want %r excess %r" % (
        what, bad.size, bad[:6], lab[bad[:6]], arg[bad[:6]],
        [float(s64[i, lab[i]] - s64[i, arg[i]] - E[i, lab[i]] - E[i, arg[i]]) if 0 <= lab[i] < s64.shape[1] else None for i in bad[:6]])
    for d in ignore:
        assert (lab != d).all(), "%s: the duplicate centroid %d was returned" % (what, d)
    amb = label_ambiguous(s64, arg, gap, E, ignore)
    ndiff = int((lab != arg).sum())
    assert ndiff <= int(amb.sum()), "%s: %d labels differ from the fp64 arg-min, only %d rows are ambiguous" % (what, ndiff, amb.sum())
    if cap is not None:
        assert amb.sum() <= cap * len(arg), "%s: %d of %d rows ambiguous: badly chosen inputs" % (what, amb.sum(), len(arg))
    return ref


# the inputs of the labelling cases: seeded, so that the CPU test of the helper sees what the GPU sees
LABEL_TILE_SCALES = (1.0, 30.0, 0.5, 20.0, 2.0, 50.0, 1.0, 10.0)      # neighbouring 128-centroid tiles differ 10-100x in norm
# (index type, kind of centroids): the large-magnitude case exists for fp16 rows only
LABEL_KINDS = [("fp32", "means"), ("fp32", "tiles"), ("fp16", "means"), ("fp16", "tiles"), ("fp16", "big")]
LABEL_NEAR_EVERY = 4                   # every 4th row of a case is moved next to the bisector of its two nearest centroids ...
LABEL_NEAR_BAND = (3.0, 30.0)          # ... to a runner-up gap of this many times E(x, arg) + E(x, runner-up)


def label_steer(cent, x, sel, metric, ignore, rng, rounds=4):
    """Moves the rows `sel` of x (in place) along c_a - c_b, a and b their two nearest centroids, until the fp64 runner-up gap
    is k (E(x, a) + E(x, b)) with k log-uniform in 6..15.  Clustered rows alone have gaps thousands of times the band, where an
    error far larger than the band flips nothing; these rows are decided by the band: a kernel whose scores are off by much
    more than 30 bands (half-precision accumulation is ~4000) labels many of them wrongly and outside the acceptance rule,
    while none is ambiguous (3 bands away at least).  The gap is linear in x along c_a - c_b (L2: 2 x.(c_a - c_b) + const,
    InnerProduct / Cosine: x.(c_a - c_b)), so one move lands on the target; it is repeated because the pair, the band and (for
    unit rows, which are renormalised) the gap change a little with the move, and because x is rounded to its own type.  That
    last rounding moves the gap by less than a band or so, which is why k stays well inside LABEL_NEAR_BAND."""
    m = _METRIC_IDS[metric]
    sel = np.asarray(sel)
    c64 = np.asarray(cent).astype(np.float64)
    dscan, dpad = label_scan_width(c64.shape[1], np.asarray(cent).dtype, m)
    c64 = c64[:, :dscan]
    if sel.size == 0 or c64.shape[0] - len(ignore) < 2:
        return
    gamma = (dpad + 8) * 2.0 ** -23
    cn2 = (c64 ** 2).sum(1)
    k = np.exp(rng.uniform(np.log(6.0), np.log(15.0), sel.size))
    for _ in range(rounds):
        xs = x[sel, :dscan].astype(np.float64)
        sc = -(xs @ c64.T) if m else cn2[None] - 2.0 * (xs @ c64.T)          # ranks the centroids; the gap itself is direct
        if len(ignore):
            sc[:, list(ignore)] = np.inf
        two = np.argpartition(sc, 1, axis=1)[:, :2]
        i = np.arange(sel.size)
        swap = sc[i, two[:, 0]] > sc[i, two[:, 1]]
        a, b = np.where(swap, two[:, 1], two[:, 0]), np.where(swap, two[:, 0], two[:, 1])
        delta = c64[a] - c64[b]
        if m == 0:
            g = ((xs - c64[b]) ** 2).sum(1) - ((xs - c64[a]) ** 2).sum(1)
            xn = np.sqrt((xs ** 2).sum(1))
            band = gamma * ((xn + np.sqrt(cn2[a])) ** 2 + (xn + np.sqrt(cn2[b])) ** 2)
        else:
            g = (xs * delta).sum(1)
            mag = (np.abs(xs) * (np.abs(c64[a]) + np.abs(c64[b]))).sum(1)
            band = gamma * mag + (2.0 ** -24 * (2.0 + mag) if m == 2 else 0.0)
        slope = (1.0 if m else 2.0) * (delta ** 2).sum(1)
        t = np.where(slope > 0, (k * band - g) / np.where(slope > 0, slope, 1.0), 0.0)
        xs += t[:, None] * delta
        if m == 2:
            xs /= np.sqrt((xs ** 2).sum(1, keepdims=True))
        x[sel, :dscan] = xs.astype(x.dtype)


def label_near_share(s64, arg, gap, E, ignore=()):
    """share of the rows whose runner-up gap is LABEL_NEAR_BAND times the band: the rows that decide"""
    if s64.shape[1] - len(ignore) < 2:
        return 0.0
    i = np.arange(len(arg))
    r = gap / (E[i, arg] + E[i, label_runner_up(s64, arg, ignore)])
    return float(((r >= LABEL_NEAR_BAND[0]) & (r <= LABEL_NEAR_BAND[1])).mean())


def label_case(rows, nlist, dim, dtype, kind, metric="SquaredEuclidean", seed=0, near=True):
    """(centroids, rows, ignore) of one labelling case: clustered Gaussians, rows = a centroid's mean + noise, every
    LABEL_NEAR_EVERY-th of them then moved next to the bisector of its two nearest centroids (label_steer; near=False: none).
    kind "means": the centroids are the means rounded to the index type; "tiles": the means of every 128-centroid tile are
    scaled by LABEL_TILE_SCALES first (a stale accumulator or norm at a tile boundary shows only when magnitudes differ);
    "big": elements up to ~1e3 (norms ~1e8: the fp32 norm path, not the half range).  With three or more centroids the last one
    is a copy of centroid 1 and is returned in `ignore`.  Cosine: unit rows followed by the norm slot(s) of the converted row."""
    npdt = np.dtype(dtype)
    m = _METRIC_IDS[metric]
    dscan, _ = label_scan_width(dim, npdt, m)
    rng = np.random.default_rng([seed, rows, nlist, dim, m, npdt.itemsize, ("means", "tiles", "big").index(kind)])
    means = rng.standard_normal((nlist, dscan))
    if kind == "tiles":
        means *= np.asarray(LABEL_TILE_SCALES)[(np.arange(nlist) // 128) % len(LABEL_TILE_SCALES)][:, None]
    if kind == "big":
        means = np.clip(means * 300.0, -900.0, 900.0)
    own = rng.integers(0, nlist, rows)
    scale = np.abs(means).mean(1, keepdims=True)[own] if dscan else 1.0
    x = means[own] + 0.3 * scale * rng.standard_normal((rows, dscan))

    def finish(a):
        if m != 2:
            return np.ascontiguousarray(a.astype(npdt))
        norm = np.sqrt((a ** 2).sum(1, keepdims=True))
        unit = (a / norm).astype(npdt)
        slot = norm.astype(np.float32)
        tail = slot.view(np.float16) if npdt == np.float16 else slot       # fp16 rows: the fp32 norm's bits in two half slots
        return np.ascontiguousarray(np.concatenate([unit, tail], 1))
    cent, x = finish(means), finish(x)
    ignore = ()
    if nlist >= 3:
        cent[nlist - 1] = cent[1]
        ignore = (nlist - 1,)
    if near:
        label_steer(cent, x, np.arange(LABEL_NEAR_EVERY - 1, rows, LABEL_NEAR_EVERY), m, ignore, rng)
    return cent, x, ignore


# (rows, centroids, dim): which step count, tile and path each shape hits is tabulated in tests/test_gpu_label_parity.py
LABEL_SHAPES = [
    (1, 1, 1), (127, 2, 31), (128, 63, 32), (129, 64, 33), (511, 127, 64), (512, 128, 65), (513, 129, 100), (767, 191, 128),
    (512, 192, 65), (513, 193, 128), (1025, 255, 129), (767, 256, 100), (511, 256, 128), (1025, 383, 31), (640, 383, 65),
    (600, 385, 129), (2500, 385, 64), (4000, 1000, 33), (2049, 1000, 100), (3000, 257, 768),
]


def label_offset_case(offset, dtype, rows=3000, nlist=256, dim=128, seed=7):
    """rows = a common offset + unit-variance spread (cluster means 0.8, noise 0.6), centroids = offset + the cluster means:
    the norm expansion |x|^2 + |c|^2 - 2 x.c cancels ~offset^2 dim to reach distances of ~dim"""
    npdt = np.dtype(dtype)
    rng = np.random.default_rng([seed, int(offset), npdt.itemsize])
    means = 0.8 * rng.standard_normal((nlist, dim))
    x = means[rng.integers(0, nlist, rows)] + 0.6 * rng.standard_normal((rows, dim))
    return np.ascontiguousarray((means + offset).astype(npdt)), np.ascontiguousarray((x + offset).astype(npdt))


def label_batch_case(rows, nlist, dim, dtype, seed=9, block=4096):
    """a row set longer than one labelling batch: a small seeded block of clustered rows, tiled, every row with its own small
    perturbation (no two rows equal), every LABEL_NEAR_EVERY-th row of every block then moved next to a bisector (label_steer).
    Block b depends on (seed, b) only: a shorter row set is a prefix of a longer one."""
    npdt = np.dtype(dtype)
    cent, blk, ignore = label_case(block, nlist, dim, np.float64, "means", seed=seed, near=False)
    cent = np.ascontiguousarray(cent.astype(npdt))
    cent[nlist - 1] = cent[1]
    x = np.empty((rows, dim), npdt)
    for o in range(0, rows, block):
        m = min(block, rows - o)
        rng = np.random.default_rng([seed, o // block])
        x[o:o + m] = (blk[:m] + 0.05 * rng.standard_normal((block, dim), dtype=np.float32)[:m]).astype(npdt)
        label_steer(cent, x[o:o + m], np.arange(LABEL_NEAR_EVERY - 1, m, LABEL_NEAR_EVERY), 0, ignore, rng)
    return cent, x, ignore


# ---- group-by reference of the fill-route tests (test_gpu_group_routes.py, test_group_reference_cpu.py) ---------------------------
IDX_NONE = 0xffffffff


def group_reference(base, queries, group_of, ngroups, gnum, gk, metric="SquaredEuclidean", threshold=None, exclude=None,
                    candidates=None):
    """Group-by search in plain fp64 (numpy only; nothing of oracle.flat_group_search is used).

    A position competes iff it is not excluded (`exclude`: bool per position), is not a hole and has group_of[pos] < ngroups.
    `candidates`: per query the positions that compete, in scan order; None = every position in storage order.  An entry of
    IDX_NONE (or any entry >= n) is a hole; a position named twice competes twice, as two candidates with their own ordinals.
    Every group keeps its gk smallest candidates under (score, scan ordinal); the groups are ordered by their best score and the
    first gnum are kept; documents with score > threshold are cut AFTER that ranking, so a group may be listed with no document.
    Scores: L2 sum((q - b)^2) summed directly, InnerProduct -q.b (label_reference's s64).

    Returns a dict
      s64, E    [nq][n]: fp64 score of every (query, position) and the per-pair bound on |dense fp32 score - s64|
      queries   per query a dict
                  groups  [(g, positions, scores)]: the listed groups in order, documents after the radius cut
                  order   {g: (scores, positions)} of EVERY admissible group: its full ascending (score, ordinal) order
                  bests   (scores, group numbers) of every admissible group, ascending (best score, group number)

    E is label_reference's bound, which holds for the flat dense pass as it stands: the scan epilogue (zvk_scan.hip.h) forms
    L2 as max(fma(-2, dot, |q|^2 + |b|^2), 0) with the dot product accumulated in fp32 on the matrix cores over the PADDED scan
    width and both norms fp32 sums of squares, InnerProduct as -dot: the very expressions E = gamma (|q| + |b|)^2 and
    E = gamma sum|q_i b_i|, gamma = (dpad + 8) 2^-23, are derived for (the clamp at 0 moves a score towards its true value)."""
    base = np.asarray(base)
    queries = np.atleast_2d(queries)
    n = base.shape[0]
    s64, _, _, E = label_reference(base, queries, metric)
    s64, E = s64.reshape(len(queries), n), E.reshape(len(queries), n)
    gof = np.asarray(group_of).astype(np.int64)
    live = gof < ngroups
    if exclude is not None:
        live &= ~np.asarray(exclude, bool)
    small = gof.astype(np.uint16) if ngroups <= 0xffff else gof      # (a stable sort of 16-bit keys is a radix sort)
    out = []
    for qi in range(len(queries)):
        if candidates is None:
            pos = np.nonzero(live)[0]
        else:
            pos = np.asarray(candidates[qi], np.int64).reshape(-1)
            pos = pos[pos < n]
            pos = pos[live[pos]]
        # pos is in scan order: two stable sorts give (group, score, ordinal)
        o1 = np.argsort(s64[qi, pos], kind="stable")
        o2 = np.argsort(small[pos[o1]], kind="stable")
        pos = pos[o1][o2]
        sc, gg = s64[qi, pos], gof[pos]
        starts = np.nonzero(np.r_[True, gg[1:] != gg[:-1]])[0] if pos.size else np.zeros(0, np.int64)
        ends = np.r_[starts[1:], pos.size]
        order = {int(gg[a]): (sc[a:b], pos[a:b]) for a, b in zip(starts, ends)}
        bg = gg[starts] if pos.size else np.zeros(0, np.int64)
        bs = sc[starts] if pos.size else np.zeros(0)
        rank = np.lexsort((bg, bs))
        groups = []
        for g in bg[rank][:gnum]:
            s, p = order[int(g)]
            s, p = s[:gk], p[:gk]
            if threshold is not None:
                keep = ~(s.astype(np.float32) > np.float32(threshold))
                s, p = s[keep], p[keep]
            groups.append((int(g), p, s))
        out.append({"groups": groups, "order": order, "bests": (bs[rank], bg[rank])})
    return {"s64": s64, "E": E, "queries": out}


def _group_places(rq, groups, ngroups_out, what):
    """the freedom of the reference's unstable sort of the groups: as many groups as the reference lists, none twice, every one
    admissible, and the group at place i has the best score the reference has at place i — so a group whose best score is
    unshared sits at its place, groups tied inside the list are all there, and the last places may hold any group with that
    best score"""
    want = rq["groups"]
    assert int(ngroups_out) == len(want), "%s: %d groups listed, reference %d" % (what, ngroups_out, len(want))
    got = [int(g) for g in groups[:len(want)]]
    assert len(set(got)) == len(got), "%s: a group is listed twice: %r" % (what, got)
    for i, g in enumerate(got):
        assert g in rq["order"], "%s place %d: group %d has no admissible member" % (what, i, g)
        assert rq["order"][g][0][0] == rq["bests"][0][i], "%s place %d: group %d (best %r), reference best %r" % (
            what, i, g, rq["order"][g][0][0], rq["bests"][0][i])
    return got


def check_groups_exact(rq, groups, ngroups_out, keys, scores, counts, gk, key_of, threshold=None, what=""):
    """one query of a group-by answer (C ABI layout: groups [gnum], keys / scores [gnum][gk], counts [gnum]) against
    group_reference on data whose scores are exact.  Lists are held exactly: the keys are key_of[the reference's first gk
    positions under (score, ordinal)], in that order, the score bits are equal and the count after the radius is equal.
    Groups: see _group_places."""
    got = _group_places(rq, groups, ngroups_out, what)
    for i, g in enumerate(got):
        s, p = rq["order"][g]
        s, p = s[:gk], p[:gk]
        if threshold is not None:
            keep = ~(s.astype(np.float32) > np.float32(threshold))
            s, p = s[keep], p[keep]
        c = int(counts[i])
        assert c == len(p), "%s group %d: %d documents, reference %d" % (what, g, c, len(p))
        wk = np.asarray(key_of)[p].astype(np.uint64)
        assert np.array_equal(np.asarray(keys[i][:c], np.uint64), wk), "%s group %d: documents\n got %r\nwant %r" % (
            what, g, np.asarray(keys[i][:c]), wk)
        gs = np.ascontiguousarray(scores[i][:c], np.float32)
        assert np.array_equal(gs.view(np.uint32), s.astype(np.float32).view(np.uint32)), "%s group %d: score bits\n got %r\nwant %r" % (
            what, g, gs, s)


def group_l2_rescore_bound(dim, s64):
    """Bound on |refined L2 score - s64|, of the form (d + c) 2^-23 s64 with c = 2.  The refinement (rescore_l2_kernel) sums the
    d squares (q_i - b_i)^2 in fp32, in a fixed tree over the lanes; the padding adds exact zeros.  With u = 2^-24: q_i - b_i
    is rounded once, so its square carries (1 + u)^2; fma(d_i, d_i, acc) multiplies exactly and rounds the sum; whatever the
    order, a term passes through at most d - 1 additions of two non-zero operands.  Every term is non-negative, so the result
    is s64 (1 + theta), |theta| <= (1 + u)^(d + 1) - 1 < (d + 2) u for d u << 1.  As for label_reference's gamma the figure is
    doubled — (d + 2) 2^-23 — which also pays for comparing an fp32 number with the fp64 one."""
    return (dim + 2) * 2.0 ** -23 * np.asarray(s64)


def check_groups_band(ref, qi, groups, ngroups_out, keys, scores, counts, gnum, gk, pos_of_key, metric, dim, what=""):
    """one query of a group-by answer on REAL-VALUED data (no radius).  With s64 / E of group_reference:
      documents  a returned document x of group g is accepted iff s64(x) - s64(gk-th of g) <= E(x) + E(gk-th); the list holds
                 min(gk, size of g) distinct admissible members of g, in ascending order of the returned score
      groups     a listed group g is accepted iff best(g) - best(gnum-th group) <= E(best doc of g) + E(best doc of the gnum-th)
      scores     L2 (re-scored directly): within group_l2_rescore_bound of s64; InnerProduct: within E
    Returns (lists that differ from the fp64 set, ambiguous lists, cut lists, group list differs, group cut ambiguous): a list
    is ambiguous when the gap between its ranks gk and gk + 1 is <= the two bounds, the group cut when the gap between the
    best scores at ranks gnum and gnum + 1 is.  Only ambiguous lists may differ: the caller sums and compares."""
    rq, s64, E = ref["queries"][qi], ref["s64"][qi], ref["E"][qi]
    bs, bg = rq["bests"]
    nlist = min(gnum, len(bg))
    assert int(ngroups_out) == nlist, "%s: %d groups listed, reference %d" % (what, ngroups_out, nlist)
    got = [int(g) for g in groups[:nlist]]
    assert len(set(got)) == len(got), "%s: a group is listed twice" % what
    ebest = lambda g: E[rq["order"][g][1][0]]
    gamb = False
    if len(bg) > gnum:
        last, nxt = int(bg[gnum - 1]), int(bg[gnum])
        gamb = bs[gnum] - bs[gnum - 1] <= ebest(last) + ebest(nxt)
    ndiff = namb = ncut = 0
    for i, g in enumerate(got):
        assert g in rq["order"], "%s place %d: group %d has no admissible member" % (what, i, g)
        s, p = rq["order"][g]
        if nlist:
            last = int(bg[nlist - 1])
            assert s[0] - bs[nlist - 1] <= ebest(g) + ebest(last), "%s: group %d (best %r) listed, rank-gnum best %r, bounds %r %r" % (
                what, g, s[0], bs[nlist - 1], ebest(g), ebest(last))
        c = int(counts[i])
        assert c == min(gk, len(p)), "%s group %d: %d documents of %d members" % (what, g, c, len(p))
        x = np.array([pos_of_key[int(k)] for k in keys[i][:c]], np.int64)
        assert len(set(x.tolist())) == c, "%s group %d: a document twice" % (what, g)
        member = set(p.tolist())
        assert all(int(v) in member for v in x), "%s group %d: a document of another group or an excluded one" % (what, g)
        kth = p[c - 1]
        exc = s64[x] - s64[kth] - E[x] - E[kth]
        assert np.all(exc <= 0), "%s group %d: document %d outside the band by %r" % (what, g, x[np.argmax(exc)], exc.max())
        gs = np.asarray(scores[i][:c], np.float64)
        assert np.all(np.diff(gs) >= 0), "%s group %d: scores not ascending" % (what, g)
        tol = group_l2_rescore_bound(dim, s64[x]) if _METRIC_IDS[metric] == 0 else E[x]
        err = np.abs(gs - s64[x])
        assert np.all(err <= tol), "%s group %d: score off by %r, bound %r" % (what, g, err.max(), tol[np.argmax(err - tol)])
        if len(p) > gk:
            ncut += 1
            namb += bool(s[gk] - s[gk - 1] <= E[p[gk]] + E[p[gk - 1]])
            ndiff += set(x.tolist()) != set(p[:gk].tolist())
    return ndiff, namb, ncut, set(got) != set(int(g) for g in bg[:nlist]), bool(gamb)
