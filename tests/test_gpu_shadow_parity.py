"""GPU tests of the half-width pre-selection (zvec_hip_*_set_shadow, zvk_shadow.hip.h) against the ORACLE — run with -m gpu.
The claim under test (include/zvec_hip.h): for every query the route through the fp16 twin returns the fp32 route's answer.
The yardstick here is the oracle, per query:
  - a query the certificate PASSED carries no selection band: its keys are the oracle's and its scores agree within rtol 2e-6 (the
    certificate speaks about true scores, so a certified query may not move inside the fp32 route's band);
  - a query answered by the fp32 rows is the fp32 route's answer (bit for bit under L2) and lies within that route's band of the oracle.
Which queries passed is read off the certify step's re-run count: flat queries go one per call (re-run 0 or 1), IVF queries as a batch
of 9 copies of one query (a batch of <= 8 takes the direct fp32 route and never touches the twin), re-run 0 or 9.  Whole batches run
as well (the 16-row and the wide tiles are different code): there a batch with no re-run carries no band."""
import ctypes as C

import numpy as np
import pytest

from tests.util import (tie_tolerant_compare, exact_l2, ivf_index, ivf_search, ivf_search_dev, flat_search, flat_search_dev)

pytestmark = pytest.mark.gpu

L2, IP = "SquaredEuclidean", "InnerProduct"


@pytest.fixture(scope="module")
def zv():
    import zvec_amd
    return zvec_amd


def _om(metric):
    from oracle import oracle as O
    return O.METRIC_L2 if metric == L2 else O.METRIC_IP


def _gamma(dim):
    return (dim + 8) * 1.1920929e-7


def _fp32_band(metric, q, base):
    """the fp32 route's selection band of every query: L2 selects on |q|^2 + |b|^2 - 2 q.b, IP reports the matrix-core
    sums; both within the accumulation error of the operand magnitudes"""
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(1))
    bn = np.sqrt((base.astype(np.float64) ** 2).sum(1)).max()
    if metric == L2:
        return 4e-6 * (2 * qn ** 2 + bn ** 2) + 1e-30
    return 4 * _gamma(q.shape[1]) * qn * bn + 1e-30


def _check(what, metric, got, ora, certified, band, fp32=None):
    """one result list set against the oracle under the rules of the module docstring"""
    gk, gs, gc = got
    ok, os_, oc = ora
    if certified:
        tie_tolerant_compare(gk, gs, gc, ok, os_, oc, rtol=2e-6, atol=1e-30, what=what + " (certified)")
    else:
        tie_tolerant_compare(gk, gs, gc, ok, os_, oc, rtol=2e-6 if metric == L2 else 1.0, atol=1e-30, scale=None if metric == L2 else band,
                             select_band=band, what=what + " (fp32)")
        if fp32 is not None and metric == L2:
            assert np.array_equal(gk, fp32[0]) and np.array_equal(gs.view(np.uint32), fp32[1].view(np.uint32)), what + ": not the fp32 route"


def _flat_pair(zv, base, metric, preselect=0):
    """the same rows twice: with the twin and without (the fp32 route)"""
    tw = zv.HipFlatSearcher(base.shape[1], metric)
    assert tw.load(base) == 0
    tw.set_shadow(True, preselect)
    ref = zv.HipFlatSearcher(base.shape[1], metric)
    assert ref.load(base) == 0
    return tw, ref


def _flat_per_query(zv, tw, ref, base, q, k, metric, oracle, what, sample=None, preselect=0, exclude_words=None):
    """queries one per call: re-run 0 / 1 is the query's certificate bit.  Returns the number certified."""
    idx = range(len(q)) if sample is None else sample
    ok, os_, _, oc = oracle.flat_search(base, q, k, metric=_om(metric), exclude_bits=exclude_words, threads=16)
    band = _fp32_band(metric, q, base)
    ctx, rctx = tw.create_context(), ref.create_context()
    ncert = 0
    for i in idx:
        tw.set_shadow(True, preselect)                       # (a fresh governor: every call goes through the twin)
        gk, gs, gc, rerun = flat_search_dev(tw, q[i:i + 1], k, ctx=ctx, exclude_words=exclude_words)
        assert rerun in (0, 1)
        fk, fs, fc, _ = flat_search_dev(ref, q[i:i + 1], k, ctx=rctx, exclude_words=exclude_words)
        _check("%s q%d" % (what, i), metric, (gk, gs, gc), (ok[i:i + 1], os_[i:i + 1], oc[i:i + 1]), rerun == 0, band[i], (fk, fs))
        ncert += rerun == 0
    return ncert


def _ivf_per_query(se, ref, cent, offs, vecs, keys, q, k, metric, oracle, what, sample, preselect=0):
    """9 copies of one query per call: re-run 0 / 9 is the query's certificate bit.  Returns the number certified."""
    nprobe, max_scan = se.probe_params()
    ok, os_, _, oc, _ = oracle.ivf_search(cent, offs, vecs, q, k, nprobe, max_scan, metric=_om(metric), keys=keys, threads=16)
    band = _fp32_band(metric, q, vecs)
    ctx, rctx = se.create_context(), ref.create_context()
    ncert = 0
    for i in sample:
        q9 = np.repeat(q[i:i + 1], 9, 0)
        se.set_shadow(True, preselect)
        gk, gs, gc, rerun = ivf_search_dev(se, q9, k, ctx=ctx)
        assert rerun in (0, 9), "%s q%d: %d of 9 copies re-run" % (what, i, rerun)
        assert all(np.array_equal(gk[0], gk[j]) for j in range(9))
        fk, fs, fc, _ = ivf_search_dev(ref, q9, k, ctx=rctx)
        _check("%s q%d" % (what, i), metric, (gk[:1], gs[:1], gc[:1]), (ok[i:i + 1], os_[i:i + 1], oc[i:i + 1]), rerun == 0, band[i],
               (fk[:1], fs[:1]))
        ncert += rerun == 0
    return ncert


def _untied(cent, q, nprobe, metric):
    """queries whose probe set is not decided by a tie of centroid scores (the oracle may break those either way)"""
    if metric == L2:
        cd = np.sort(exact_l2(cent, q), 1)
    else:
        cd = np.sort(-(q.astype(np.float64) @ cent.astype(np.float64).T), 1)
    if nprobe >= cd.shape[1]:
        return np.arange(len(q))
    return np.nonzero(cd[:, nprobe - 1] != cd[:, nprobe])[0]


def _ivf_pair(rng, base, nlist, metric, ratio):
    se, cent, offs, vecs, keys = ivf_index(rng, base, nlist, metric=metric, ratio=ratio)
    import zvec_amd
    ref = zvec_amd.HipIVFSearcher(base.shape[1], metric, scan_ratio=ratio, brute_force_threshold=10)
    assert ref.load(cent, offs, vecs, keys) == 0
    se.set_shadow(True)
    return se, ref, cent, offs, vecs, keys


def _batch_vs_oracle(what, metric, got, rerun, ora, band, sel=None):
    gk, gs, gc = got
    ok, os_, oc = ora
    if sel is not None:
        gk, gs, gc, ok, os_, oc = gk[sel], gs[sel], gc[sel], ok[sel], os_[sel], oc[sel]
        band = band[sel]
    if rerun and metric == IP:      # (scores of the queries the fp32 route answered: its matrix-core sums, within its band)
        tie_tolerant_compare(gk, gs, gc, ok, os_, oc, rtol=1.0, atol=1e-30, scale=band, select_band=band, what=what)
    else:
        tie_tolerant_compare(gk, gs, gc, ok, os_, oc, rtol=2e-6, atol=1e-30, select_band=band if rerun else None, what=what)


def _clustered(rng, n, dim, nq, noise, nc=None, scale=6.0, with_centres=False):
    nc = nc or max(4, n // 400)
    centres = rng.standard_normal((nc, dim)).astype(np.float32) * scale
    base = (centres[rng.integers(0, nc, n)] + noise * scale * rng.standard_normal((n, dim))).astype(np.float32)
    q = (centres[rng.integers(0, nc, nq)] + noise * scale * rng.standard_normal((nq, dim))).astype(np.float32)
    return (base, q, centres) if with_centres else (base, q)


# ---- 1. inner product at the rounding scale ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("noise", [1e-3, 1e-2, 0.03, 0.1, 0.3])
def test_ip_at_the_rounding_scale(zv, oracle, noise, outliers):
    """the sweep of test_certificate_at_the_rounding_scale under inner product; with 1 % of the rows at 30-100x the median norm the IP
    bound (max-over-rows facts: |q - q16| max|b16|) is at its loosest.  Those rows point away from every cluster (orthogonal to the
    centres), so they never enter a result but set max|b16|: heavy re-runs, and the governor suspends the route — the answers stay
    the oracle's"""
    rng = np.random.default_rng(int(noise * 1e6) + 7 * outliers)
    dim, nlist, k, per = 96, 12, 10, 400
    base, q, centres = _clustered(rng, nlist * per, dim, 48, noise, nc=nlist, with_centres=True)
    if outliers:
        rows = rng.choice(len(base), len(base) // 100, replace=False)
        basis = np.linalg.qr(centres.T.astype(np.float64))[0]
        d = rng.standard_normal((len(rows), dim))
        d -= (d @ basis) @ basis.T                         # (orthogonal to the centres: the queries' dots with them stay small)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        med = np.median(np.linalg.norm(base, axis=1))
        base[rows] = (d * med * rng.uniform(30, 100, (len(rows), 1))).astype(np.float32)
    tw, ref = _flat_pair(zv, base, IP)
    nc = _flat_per_query(zv, tw, ref, base, q, k, IP, oracle, "flat ip noise %g" % noise, sample=range(16))
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, nlist, IP, 0.3)
    nprobe, max_scan = se.probe_params()
    sel = _untied(cent, q, nprobe, IP)
    ni = _ivf_per_query(se, iref, cent, offs, vecs, keys, q, k, IP, oracle, "ivf ip noise %g" % noise, sel[:8])
    # whole batches (the 16-row / wide tiles), several in a row: with the outliers the governor may suspend the twin (the suspended
    # searches read the fp32 rows: inside that route's band)
    ok, os_, _, oc = oracle.flat_search(base, q, k, metric=_om(IP), threads=16)
    band = _fp32_band(IP, q, base)
    tw.set_shadow(True)
    reruns, suspended = [], False
    for step in range(6):
        gk, gs, gc, rerun = flat_search_dev(tw, q, k)
        reruns.append(rerun)
        suspended = suspended or (step >= 4 and all(r * 2 > len(q) for r in reruns[step - 4:step]))
        _batch_vs_oracle("flat ip batch noise %g step %d" % (noise, step), IP, (gk, gs, gc), rerun or suspended, (ok, os_, oc), band)
    iok, ios, _, ioc, _ = oracle.ivf_search(cent, offs, vecs, q, k, nprobe, max_scan, metric=_om(IP), keys=keys, threads=16)
    gk, gs, gc, irerun = ivf_search_dev(se, q, k)
    _batch_vs_oracle("ivf ip batch noise %g" % noise, IP, (gk, gs, gc), irerun, (iok, ios, ioc), _fp32_band(IP, q, vecs), sel)
    print("ip noise %g outliers %s: flat certified %d of 16, ivf %d of %d; batch re-runs flat %s ivf %d of 48"
          % (noise, outliers, nc, ni, min(8, len(sel)), reruns, irerun))
    if outliers and noise <= 0.1:
        # |q - q16| max|b16| ~ 1e2 against gaps of a few units between the k-th and the k'-th dot: (nearly) every query re-runs, four
        # such batches suspend the twin, the next ones read the fp32 rows (nothing re-run)
        assert all(r * 2 > len(q) for r in reruns[:4]) and suspended and reruns[4] == 0, reruns


def _biased_query_rows(rng, nq, dim, far=3000):
    """IP: rows exact in fp16 (|b - b16| = 0); queries whose fp32 values sit 0.45 ulp off their fp16 image, so that the query's rounding
    e = q - q16 is a fixed direction.  Per query: 10 unit rows K with fp16 dot X (true dot the same up to e.b, small for them), one row
    T at X - 5e-4 and 10 rows A at X - 7e-4 whose component along e makes their TRUE dot about X + 2e-4.  k' = k + 1 keeps K and T: the
    A rows, truly the best, are left out, and only the query-rounding term |q - q16| max|b16| of the bound stops that from being
    certified (the accumulation terms alone would pass it)"""
    qs, rows = [], []
    for _ in range(nq):
        q16 = (rng.uniform(0.25, 0.5, dim) * rng.choice([-1.0, 1.0], dim)).astype(np.float16)
        up = np.abs(np.nextafter(q16, np.float16(np.inf)).astype(np.float64) - q16)
        dn = np.abs(q16.astype(np.float64) - np.nextafter(q16, np.float16(-np.inf)))
        q = (q16.astype(np.float64) + 0.45 * np.minimum(up, dn) * rng.choice([-1.0, 1.0], dim)).astype(np.float32)
        assert np.array_equal(q.astype(np.float16), q16)
        qd = q16.astype(np.float64)
        e = q.astype(np.float64) - qd
        w = qd / np.linalg.norm(qd)
        v = e - (e @ w) * w
        v /= np.linalg.norm(v)
        X = 0.5 * np.linalg.norm(qd)                       # fp16 dot of a unit row at 60 degrees from q16

        def unit_rows(n, dot16, along_v):
            u = rng.standard_normal((n, dim))
            u -= np.outer(u @ w, w) + np.outer(u @ v, v)
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            a = np.full(n, dot16 / np.linalg.norm(qd))
            rest = np.sqrt(np.maximum(1.0 - a ** 2 - along_v ** 2, 0.0))
            return (a[:, None] * w + along_v * v + rest[:, None] * u).astype(np.float16).astype(np.float32)
        rows += [unit_rows(10, X, 0.0), unit_rows(1, X - 5e-4, 0.0), unit_rows(10, X - 7e-4, 0.85)]
        qs.append(q)
    bg = rng.standard_normal((far, dim))
    rows.append((bg / np.linalg.norm(bg, axis=1, keepdims=True)).astype(np.float16).astype(np.float32))
    return np.concatenate(rows).astype(np.float32), np.array(qs, np.float32)


def test_ip_certificate_allows_for_the_query_rounding(zv, oracle):
    rng = np.random.default_rng(89)
    nq, dim, k = 16, 96, 10
    base, q = _biased_query_rows(rng, nq, dim)
    assert _flat_pair(zv, base, IP)[0].shadow_info()["max_row_error"] == 0.0
    tw, ref = _flat_pair(zv, base, IP, k + 1)
    nc = _flat_per_query(zv, tw, ref, base, q, k, IP, oracle, "flat biased query rounding", preselect=k + 1)
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, 4, IP, 1.0)
    ni = _ivf_per_query(se, iref, cent, offs, vecs, keys, q, k, IP, oracle, "ivf biased query rounding", range(6), preselect=k + 1)
    print("biased query rounding (ip), k' = k + 1: flat certified %d of %d, ivf %d of 6" % (nc, nq, ni))


@pytest.mark.parametrize("noise", [1e-3, 3e-3, 1e-2])
def test_l2_at_the_rounding_scale_with_half_exact_queries(zv, oracle, noise):
    """queries that are exact in fp16 (|q - q16| = 0): the rows' own rounding (max |b - b16|) is then the whole of what separates the
    fp16 ranking from the true one, and the certificate must allow for it — at k' = k + 1 the k-th and the k'-th rows lie at the
    rounding scale of each other"""
    rng = np.random.default_rng(int(noise * 1e5) + 13)
    dim, nlist, k, per = 96, 12, 10, 400
    base, q = _clustered(rng, nlist * per, dim, 48, noise, nc=nlist)
    q = q.astype(np.float16).astype(np.float32)
    tw, ref = _flat_pair(zv, base, L2)
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, nlist, L2, 0.3)
    sel = _untied(cent, q, se.probe_params()[0], L2)
    for pre in (k + 1, 0):
        nc = _flat_per_query(zv, tw, ref, base, q, k, L2, oracle, "flat l2 half-exact noise %g pre %d" % (noise, pre), sample=range(24),
                             preselect=pre)
        ni = _ivf_per_query(se, iref, cent, offs, vecs, keys, q, k, L2, oracle, "ivf l2 half-exact noise %g pre %d" % (noise, pre), sel[:8],
                            preselect=pre)
        print("l2 half-exact queries, noise %g, k' %d: flat certified %d of 24, ivf %d of %d" % (noise, pre, nc, ni, min(8, len(sel))))


def _biased_rounding_rows(rng, nq, dim, far=3000):
    """queries exact in fp16; around each, 10 fp16-exact rows at distance 1, one more at 1.0005 and 12 rows A whose fp16 images lie at
    1.0010 but whose fp32 values sit 0.45 ulp off those images TOWARD the query (truly nearer than 1).  A width of k + 1 keeps the 11
    exact rows: the A rows are left out with shadow scores beyond the 11th, and only the rows' measured rounding (max |b - b16|) stops
    that from being certified"""
    def on_grid(h, q, pull):
        h16 = h.astype(np.float16)
        up = np.abs(np.nextafter(h16, np.float16(np.inf)).astype(np.float64) - h16)
        dn = np.abs(h16.astype(np.float64) - np.nextafter(h16, np.float16(-np.inf)))
        b = (h16.astype(np.float64) + pull * 0.45 * np.minimum(up, dn) * np.sign(q.astype(np.float64) - h16)).astype(np.float32)
        assert np.array_equal(b.astype(np.float16), h16)
        return b
    q = rng.standard_normal((nq, dim))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * 3.6).astype(np.float16).astype(np.float32)
    rows = []
    for i in range(nq):
        for radii, pull in (([1.0] * 10 + [1.0005], 0.0), ([1.0010] * 12, 1.0)):
            u = rng.standard_normal((len(radii), dim))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            rows.append(on_grid(q[i].astype(np.float64) + np.array(radii)[:, None] * u, q[i], pull))
    bg = rng.standard_normal((far, dim))
    rows.append((bg / np.linalg.norm(bg, axis=1, keepdims=True) * 3.6).astype(np.float32))
    return np.concatenate(rows).astype(np.float32), q


def test_l2_certificate_allows_for_the_row_rounding(zv, oracle):
    rng = np.random.default_rng(97)
    nq, dim, k = 16, 96, 10
    base, q = _biased_rounding_rows(rng, nq, dim)
    tw, ref = _flat_pair(zv, base, L2, k + 1)
    nc = _flat_per_query(zv, tw, ref, base, q, k, L2, oracle, "flat biased rounding", preselect=k + 1)
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, 4, L2, 1.0)
    ni = _ivf_per_query(se, iref, cent, offs, vecs, keys, q, k, L2, oracle, "ivf biased rounding", range(6), preselect=k + 1)
    print("biased row rounding, k' = k + 1: flat certified %d of %d, ivf %d of 6" % (nc, nq, ni))


# ---- 2. fp16 subnormals ------------------------------------------------------------------------------------------------------------
def _subnormal_data(rng, n, nq, dim, case):
    """elements in 1e-7..6e-5 (fp16 subnormals) mixed with O(1) ones; `only`: the rows differ from each other only in such elements;
    `tiny`: every element is one (the dot products of the scan consist of subnormal products alone)"""
    def small(shape):
        return (rng.uniform(1e-7, 6e-5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if case == "mixed":
        x = rng.standard_normal((n + nq, dim)).astype(np.float32)
        m = rng.random((n + nq, dim)) < rng.uniform(0.3, 0.6, (n + nq, 1))
        x[m] = small(int(m.sum()))
    elif case == "only":
        common = rng.standard_normal(dim).astype(np.float32)
        sub = rng.random(dim) < 0.5
        x = np.tile(common, (n + nq, 1))
        x[:, sub] = small((n + nq, int(sub.sum())))
    else:
        x = small((n + nq, dim))
    return x[:n].copy(), x[n:].copy()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("case", ["mixed", "only", "tiny"])
def test_subnormal_elements(zv, oracle, metric, case):
    rng = np.random.default_rng(101 + ["mixed", "only", "tiny"].index(case) + 10 * (metric == IP))
    n, dim, nq, k = 12000, 64, 40, 10
    base, q = _subnormal_data(rng, n, nq, dim, case)
    tw, ref = _flat_pair(zv, base, metric)
    nc = _flat_per_query(zv, tw, ref, base, q, k, metric, oracle, "flat subnormal %s %s" % (case, metric), sample=range(20))
    ok, os_, _, oc = oracle.flat_search(base, q, k, metric=_om(metric), threads=16)
    tw.set_shadow(True)
    gk, gs, gc, rerun = flat_search_dev(tw, q, k)
    _batch_vs_oracle("flat subnormal batch %s %s" % (case, metric), metric, (gk, gs, gc), rerun, (ok, os_, oc), _fp32_band(metric, q, base))
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, 16, metric, 0.25)
    nprobe, _ = se.probe_params()
    sel = _untied(cent, q, nprobe, metric)
    ni = _ivf_per_query(se, iref, cent, offs, vecs, keys, q, k, metric, oracle, "ivf subnormal %s %s" % (case, metric), sel[:6])
    print("subnormal %s %s: flat certified %d of 20 (batch re-ran %d of %d), ivf certified %d of %d"
          % (case, metric, nc, rerun, nq, ni, min(6, len(sel))))
    # `tiny` decides whether the f16 matrix cores keep fp16 subnormals: if they flushed them, every dot product of the scan would be 0,
    # the pre-selection would follow |b|^2 alone and the certified answers would not be the oracle's.  So it (and `mixed`) must
    # certify most queries.  `only` cannot certify: the rows' differences (~1e-9 in squared distance) lie far below the accumulation
    # bound (~1e-5 (|q|^2 + |b|^2)) — it checks the re-run path with subnormal-only differences.
    if case != "only":
        assert nc >= 15 and ni >= min(4, len(sel)), "subnormal %s %s: only %d of 20 / %d certified" % (case, metric, nc, ni)


# ---- 3. shapes and widths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 33, 65, 100, 129, 768])
def test_flat_shapes_and_widths(zv, oracle, dim):
    """fp16 padding to 64 elements with odd tails; k 1 / 10 / 32 at the index's width, k + 1 and 64; a width <= k and k = 33 bypass the
    twin (the fp32 route answers, nothing flagged); batches of 1 / 8 / 65 / 300 (16-row shape, narrow tile, wide 8-wave tile)"""
    rng = np.random.default_rng(dim)
    n = 20000
    base, q = _clustered(rng, n, dim, 300, 0.15)
    tw, ref = _flat_pair(zv, base, L2)
    nc = 0
    for k in (1, 10, 32):
        for pre in (0, k + 1, 64):
            nc += _flat_per_query(zv, tw, ref, base, q, k, L2, oracle, "flat d%d k%d pre%d" % (dim, k, pre), sample=range(3), preselect=pre)
    assert nc >= 9                                              # (the certificate path itself is exercised)
    ok, os_, _, oc = oracle.flat_search(base, q, 10, threads=16)
    band = _fp32_band(L2, q, base)
    tw.set_shadow(True)
    for nq in (1, 8, 65, 300):
        gk, gs, gc, rerun = flat_search_dev(tw, q[:nq], 10)
        _batch_vs_oracle("flat d%d batch %d" % (dim, nq), L2, (gk, gs, gc), rerun, (ok[:nq], os_[:nq], oc[:nq]), band[:nq])
        hk, hs, hc = flat_search(tw, q[:nq], 10)                # host pointers: certified inside the call
        _batch_vs_oracle("flat d%d host batch %d" % (dim, nq), L2, (hk, hs, hc), 1, (ok[:nq], os_[:nq], oc[:nq]), band[:nq])
    # the twin bypassed: k = 33, a width <= k
    for k, pre in ((33, 0), (10, 8)):
        tw.set_shadow(True, pre)
        gk, gs, gc, rerun = flat_search_dev(tw, q[:65], k)
        fk, fs, fc, _ = flat_search_dev(ref, q[:65], k)
        assert rerun == 0
        assert np.array_equal(gk, fk) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32)) and np.array_equal(gc, fc)


@pytest.mark.parametrize("ratio", [0.02, 0.1, 0.5, 1.0])
def test_ivf_shapes_and_scan_ratios(zv, oracle, ratio):
    """scan ratios from a couple of lists to all of them (max_scan_count cuts the last probed list mid-list), empty lists; odd dims;
    batches of <= 8 take the direct fp32 route (re-run 0, the fp32 route's answer)"""
    rng = np.random.default_rng(int(ratio * 100))
    for dim in (33, 129):
        n, nlist = 12000, 40
        base, q = _clustered(rng, n, dim, 300, 0.15, nc=30)
        se, ref, cent, offs, vecs, keys = _ivf_pair(rng, base, nlist, L2, ratio)
        # two empty lists: centroids no row is nearest to
        cent2 = np.concatenate([cent, np.full((2, dim), 1e3, np.float32)])
        offs2 = np.concatenate([offs, [offs[-1], offs[-1]]]).astype(np.uint64)
        se2 = zv.HipIVFSearcher(dim, L2, scan_ratio=ratio, brute_force_threshold=10)
        assert se2.load(cent2, offs2, vecs, keys) == 0
        se2.set_shadow(True)
        for idx, (s, c_, o_) in enumerate(((se, cent, offs), (se2, cent2, offs2))):
            nprobe, max_scan = s.probe_params()
            ok, os_, _, oc, _ = oracle.ivf_search(c_, o_, vecs, q, 10, nprobe, max_scan, keys=keys, threads=16)
            sel = _untied(c_, q, nprobe, L2)
            band = _fp32_band(L2, q, vecs)
            for nq in (9, 65, 300):
                s.set_shadow(True)
                gk, gs, gc, rerun = ivf_search_dev(s, q[:nq], 10)
                sq = sel[sel < nq]
                _batch_vs_oracle("ivf r%g d%d lists%d batch %d" % (ratio, dim, idx, nq), L2, (gk, gs, gc), rerun,
                                 (ok[:nq], os_[:nq], oc[:nq]), band[:nq], sq)
        sel = _untied(cent, q, se.probe_params()[0], L2)
        nc = _ivf_per_query(se, ref, cent, offs, vecs, keys, q, 10, L2, oracle, "ivf r%g d%d" % (ratio, dim), sel[:3])
        for k, pre in ((1, 0), (32, 33), (10, 64)):
            _ivf_per_query(se, ref, cent, offs, vecs, keys, q, k, L2, oracle, "ivf r%g d%d k%d pre%d" % (ratio, dim, k, pre), sel[:2], pre)
        # the direct route, k = 33, a width <= k: the fp32 route's answer, nothing re-run
        for nq, k, pre in ((1, 10, 0), (8, 10, 0), (65, 33, 0), (65, 10, 8)):
            se.set_shadow(True, pre)
            gk, gs, gc, rerun = ivf_search_dev(se, q[:nq], k)
            fk, fs, fc, _ = ivf_search_dev(ref, q[:nq], k)
            assert rerun == 0
            assert np.array_equal(gk, fk) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32)) and np.array_equal(gc, fc)
        print("ivf ratio %g dim %d: %d of 3 certified" % (ratio, dim, nc))


# ---- 4. filters on the twin --------------------------------------------------------------------------------------------------------
def _keep_words(rng, n, keep, kp=32):
    if keep == "few":
        kept = rng.choice(n, kp // 2, replace=False)
        mask = np.ones(n, bool)
        mask[kept] = False
    else:
        mask = rng.random(n) >= keep
    from oracle.oracle import pack_bits
    return pack_bits(mask)


def _profiled_search_dev(tw, q, k, words):
    """flat_search_dev on a profiling context; also returns the rows the scan over the twin read per query (its recorded flops /
    (2 x queries x dims)): every stored row for the dense exclude set, the kept rows for the gather variant, 0 for none"""
    ctx = tw.create_context()
    ctx.profile(True)
    gk, gs, gc, rerun = flat_search_dev(tw, q, k, ctx=ctx, exclude_words=words)
    p = ctx.profile_read()
    return (gk, gs, gc), rerun, p["flops"] / (2.0 * len(q) * q.shape[1])


@pytest.mark.parametrize("keep", [0.9, 0.5, 0.1, 0.02, "few", 0.0])
def test_flat_filters_on_the_twin(zv, oracle, keep):
    """sparse keep-sets over the twin (flat_scan_prepared, api_flat_scan.inc.h): the twin can only take the gather variant (its
    positions are stored positions), which needs a wide batch — > 2 x QGROUP = 64 queries, pick_ng == 4 — a width whose lists fit
    scan8_lds_bytes, and at most 0.9 of the rows kept; 64 queries scan every row under the dense exclude set.  Which one ran is read
    back from the scan's recorded work, so a change of those thresholds cannot silently drop either path from this test."""
    rng = np.random.default_rng(int(np.float64(0.0 if keep == "few" else keep) * 1000) + 3)
    n, dim, k = 70000, 64, 10
    base, q = _clustered(rng, n, dim, 130, 0.2)
    words = _keep_words(rng, n, keep)
    tw, ref = _flat_pair(zv, base, L2)
    ok, os_, _, oc = oracle.flat_search(base, q, k, exclude_bits=words, threads=16)
    band = _fp32_band(L2, q, base)
    kept = n - int(sum(bin(int(x)).count("1") for x in words))
    reruns, paths = [], []
    for pre in (0, 64):
        for nq in (64, 130):
            tw.set_shadow(True, pre)
            (gk, gs, gc), rerun, rows = _profiled_search_dev(tw, q[:nq], k, words)
            if rerun == 0:                                   # (re-runs add scans of their own)
                may_gather = nq > 64 and kept <= 0.9 * n
                want = (kept,) if may_gather and pre == 0 else (kept, n) if may_gather else (n,)
                assert rows in want, "keep %s pre %d batch %d: the scan read %g rows per query (%d kept of %d)" % (keep, pre, nq, rows, kept, n)
                paths.append("gather" if rows == kept else "dense")
            _batch_vs_oracle("flat keep %s pre %d batch %d" % (keep, pre, nq), L2, (gk, gs, gc), rerun, (ok[:nq], os_[:nq], oc[:nq]), band[:nq])
            hk, hs, hc = flat_search(tw, q[:nq], k, exclude_words=words)
            _batch_vs_oracle("flat host keep %s pre %d batch %d" % (keep, pre, nq), L2, (hk, hs, hc), 1, (ok[:nq], os_[:nq], oc[:nq]),
                             band[:nq])
            reruns.append(rerun)
    _flat_per_query(zv, tw, ref, base, q, k, L2, oracle, "flat keep %s" % keep, sample=range(3), exclude_words=words)
    print("flat keep %s: batch re-runs %s, paths %s" % (keep, reruns, paths))


def test_flat_seeded_gather_on_the_twin(zv, oracle):
    """>= 262 144 kept rows (64 x SEED_ROWS) and k' <= 64: flat_scan_gather seeds its bounds from a prefix of the kept fp16 rows before
    the gathered scan (the seed pass itself is not recorded; that the gathered scan ran, and over how many rows, is)"""
    rng = np.random.default_rng(600)
    n, dim, k, nq = 600000, 64, 10, 130
    base, q = _clustered(rng, n, dim, nq, 0.2, nc=300)
    words = _keep_words(rng, n, 0.5)
    tw = zv.HipFlatSearcher(dim, L2)
    assert tw.load(base) == 0
    tw.set_shadow(True)
    ok, os_, _, oc = oracle.flat_search(base, q, k, exclude_bits=words, threads=16)
    kept = n - int(sum(bin(int(x)).count("1") for x in words))
    assert kept >= 64 * 4096 and tw.shadow_width(k) <= 64
    (gk, gs, gc), rerun, rows = _profiled_search_dev(tw, q, k, words)
    assert rerun > 0 or rows == kept, "the scan over the twin read %g rows per query, not the %d kept" % (rows, kept)
    _batch_vs_oracle("flat seeded gather", L2, (gk, gs, gc), rerun, (ok, os_, oc), _fp32_band(L2, q, base))
    print("seeded gather: re-ran %d of %d" % (rerun, nq))


@pytest.mark.parametrize("keep", [0.5, 0.1, "few"])
def test_ivf_filters_on_the_twin(zv, oracle, keep):
    rng = np.random.default_rng(int(np.float64(0.0 if keep == "few" else keep) * 1000) + 5)
    n, dim, nlist, k = 20000, 48, 32, 10
    base, q = _clustered(rng, n, dim, 130, 0.2, nc=40)
    se, ref, cent, offs, vecs, keys = _ivf_pair(rng, base, nlist, L2, 0.2)
    words = _keep_words(rng, n, keep)
    nprobe, max_scan = se.probe_params()
    ok, os_, _, oc, _ = oracle.ivf_search(cent, offs, vecs, q, k, nprobe, max_scan, keys=keys, exclude_bits=words, threads=16)
    sel = _untied(cent, q, nprobe, L2)
    band = _fp32_band(L2, q, vecs)
    for nq in (9, 130):
        se.set_shadow(True)
        gk, gs, gc, rerun = ivf_search_dev(se, q[:nq], k, exclude_words=words)
        _batch_vs_oracle("ivf keep %s batch %d" % (keep, nq), L2, (gk, gs, gc), rerun, (ok[:nq], os_[:nq], oc[:nq]), band[:nq], sel[sel < nq])
        hk, hs, hc = ivf_search(se, q[:nq], k, exclude_words=words)
        _batch_vs_oracle("ivf host keep %s batch %d" % (keep, nq), L2, (hk, hs, hc), 1, (ok[:nq], os_[:nq], oc[:nq]), band[:nq], sel[sel < nq])


# ---- 5. the second pass ------------------------------------------------------------------------------------------------------------
def _near_rows(rng, nq, dim, per, far=3000):
    """every query has `per` rows within the fp16 rounding of it (distinct in fp32, ~1e-5..2e-4 of its norm away); the rest is far"""
    q = (rng.standard_normal((nq, dim)) * 4).astype(np.float32)
    near = []
    for i in range(nq):
        d = rng.standard_normal((per, dim))
        d *= (np.linspace(1e-5, 2e-4, per) * np.linalg.norm(q[i]) / np.linalg.norm(d, axis=1))[:, None]
        near.append((q[i] + d).astype(np.float32))
    bg = (rng.standard_normal((far, dim)) * 4).astype(np.float32)
    base = np.concatenate(near + [bg]).astype(np.float32)
    assert len(np.unique(base, axis=0)) == len(base)
    return base, q


@pytest.mark.parametrize("per,preselect,want", [(20, 16, "second"), (40, 16, "fp32"), (80, 64, "fp32")])
def test_second_pass(zv, oracle, per, preselect, want):
    """20 rows within the rounding: k' = 16 cannot certify, the 32-row second pass does (nothing re-run in fp32); 40 such rows defeat
    the second pass too; at k' = 64 there is no second pass"""
    rng = np.random.default_rng(per + preselect)
    nq, dim, k = 24, 64, 10
    base, q = _near_rows(rng, nq, dim, per)
    ok, os_, _, oc = oracle.flat_search(base, q, k, threads=16)
    expect = 0 if want == "second" else nq
    tw, ref = _flat_pair(zv, base, L2, preselect)
    gk, gs, gc, rerun = flat_search_dev(tw, q, k)
    assert rerun == expect, "flat: %d of %d re-run in fp32" % (rerun, nq)
    _batch_vs_oracle("flat second pass %d/%d" % (per, preselect), L2, (gk, gs, gc), rerun, (ok, os_, oc), _fp32_band(L2, q, base))
    tw.set_shadow(True, preselect)
    hk, hs, hc = flat_search(tw, q, k)
    assert np.array_equal(hk, gk) and np.array_equal(hs.view(np.uint32), gs.view(np.uint32))
    # IVF: all rows of a query in one list, every list probed
    se, iref, cent, offs, vecs, keys = _ivf_pair(rng, base, 8, L2, 1.0)
    se.set_shadow(True, preselect)
    nprobe, max_scan = se.probe_params()
    iok, ios, _, ioc, _ = oracle.ivf_search(cent, offs, vecs, q, k, nprobe, max_scan, keys=keys, threads=16)
    gk, gs, gc, irerun = ivf_search_dev(se, q, k)
    assert irerun == expect, "ivf: %d of %d re-run in fp32" % (irerun, nq)
    _batch_vs_oracle("ivf second pass %d/%d" % (per, preselect), L2, (gk, gs, gc), irerun, (iok, ios, ioc), _fp32_band(L2, q, vecs))
    se.set_shadow(True, preselect)
    hk, hs, hc = ivf_search(se, q, k)
    assert np.array_equal(hk, gk) and np.array_equal(hs.view(np.uint32), gs.view(np.uint32))
    print("second pass, %d near rows, k' %d: re-run in fp32 flat %d ivf %d of %d" % (per, preselect, rerun, irerun, nq))


# ---- 6. context state --------------------------------------------------------------------------------------------------------------
def _buffers(q, k):
    """device queries + result arrays of a search whose certify step the test runs itself"""
    import torch
    from tests.util import dev_lists
    dq, keys, scores, counts, _ = dev_lists(q, k, None)
    torch.cuda.synchronize()
    return dq, keys, scores, counts


def test_context_state(zv):
    import torch
    from zvec_amd import _lib
    rng = np.random.default_rng(61)
    n, dim, nq, k = 20000, 32, 70, 10
    base, q = _near_rows(rng, nq, dim, 40, far=n)       # every query fails its certificate: a certify step has work to do
    fl = zv.HipFlatStreamer(dim, L2)
    assert fl.add_batch(base) == 0
    fl.set_shadow(True, 16)
    ref = zv.HipFlatSearcher(dim, L2)
    assert ref.load(base) == 0
    fk, fs, fc, _ = flat_search_dev(ref, q, k)
    ctx = fl.create_context()

    # 1. a pending search, then search_by_ids / grouped searches / batch_distance on the same context: nothing is pending any more
    for other in ("by_ids", "grouped", "grouped_by_ids", "batch_distance"):
        fl.set_shadow(True, 16)
        dq, keys, scores, counts = _buffers(q, k)
        assert fl.search_dev(dq.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx) == 0
        torch.cuda.synchronize()
        if other == "by_ids":
            ctx.set_topk(k)
            assert fl.search_bf_by_p_keys_impl(q, [[1, 2, 3]] * nq, nq, ctx) == 0
        elif other == "batch_distance":
            fl.batch_distance(q[0], [0, 1, 2], ctx)
        else:
            ctx.set_group_params(2, 3)
            ctx.set_group_by(lambda key: int(key) % 2)
            p = None if other == "grouped" else [[1, 2, 3]] * nq
            assert (fl.search_impl(q, nq, ctx) if p is None else fl.search_bf_by_p_keys_impl(q, p, nq, ctx)) == 0
            ctx.reset_group_by()
        mk = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        ms = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        mc = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
        assert fl.shadow_certify(dq.data_ptr(), nq, k, mk.data_ptr(), ms.data_ptr(), mc.data_ptr(), ctx) == 0, other
        torch.cuda.synchronize()
        assert (mk == 7).all() and (ms == 7.0).all() and (mc == 7).all(), other + ": the certify step wrote over the caller's arrays"

    # 2. one context, a flat and an IVF index: the certify step of the other index is refused, the right one then completes
    se, iref, cent, offs, vecs, ikeys = _ivf_pair(rng, base, 16, L2, 0.5)
    se.set_shadow(True, 16)
    nprobe, max_scan = se.probe_params()
    ik, is_, ic, _ = ivf_search_dev(iref, q, k)
    bad = zv.IndexError_.InvalidArgument
    L = _lib.lib()
    rr = C.c_uint32(0)

    def flat_certify(dq, keys, scores, counts, topk=k):
        return L.zvec_hip_flat_shadow_certify(fl._h, ctx._h, C.c_void_p(dq.data_ptr()), nq, topk, None, C.c_void_p(keys.data_ptr()),
                                              C.c_void_p(scores.data_ptr()), C.c_void_p(counts.data_ptr()), None, C.byref(rr))

    def ivf_certify(dq, keys, scores, counts, topk=k):
        return L.zvec_hip_ivf_shadow_certify(se._h, ctx._h, C.c_void_p(dq.data_ptr()), nq, topk, nprobe, max_scan, None,
                                             C.c_void_p(keys.data_ptr()), C.c_void_p(scores.data_ptr()), C.c_void_p(counts.data_ptr()),
                                             None, C.byref(rr))

    # a pending IVF search: flat's certify is refused, IVF's completes
    dq, keys, scores, counts = _buffers(q, k)
    assert se.search_dev(dq.data_ptr(), nq, k, nprobe, max_scan, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx) == 0
    assert flat_certify(dq, keys, scores, counts) == bad
    assert ivf_certify(dq, keys, scores, counts, topk=k - 1) == bad          # 3. another k
    assert ivf_certify(dq, keys, scores, counts) == 0 and rr.value > 0
    torch.cuda.synchronize()
    gk, gs, gc = keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)
    assert np.array_equal(gk, ik) and np.array_equal(gs.view(np.uint32), is_.view(np.uint32)) and np.array_equal(gc, ic)
    # and the reverse
    fl.set_shadow(True, 16)
    dq, keys, scores, counts = _buffers(q, k)
    assert fl.search_dev(dq.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx) == 0
    assert ivf_certify(dq, keys, scores, counts) == bad
    assert flat_certify(dq, keys, scores, counts, topk=k - 1) == bad           # (a smaller k: the arrays stay in bounds either way)
    assert flat_certify(dq, keys, scores, counts) == 0 and rr.value == nq
    torch.cuda.synchronize()
    gk, gs, gc = keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)
    assert np.array_equal(gk, fk) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32)) and np.array_equal(gc, fc)

    # 4. the twin dropped between the search and its certify step: the step still completes, with the fp32 route's answer
    fl.set_shadow(True, 16)
    dq, keys, scores, counts = _buffers(q, k)
    assert fl.search_dev(dq.data_ptr(), nq, k, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx) == 0
    fl.set_shadow(False)
    assert flat_certify(dq, keys, scores, counts) == 0 and rr.value == nq
    torch.cuda.synchronize()
    gk, gs, gc = keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)
    assert np.array_equal(gk, fk) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32)) and np.array_equal(gc, fc)


# ---- 7. twin staleness -------------------------------------------------------------------------------------------------------------
def _blocks(rows, keys, bvc=32):
    """FlatStreamerEntity's persisted blocks: [bvc rows][bvc u64 keys][DeletionMap 4 B][BlockHeader 12 B], every row live"""
    n, dim = rows.shape
    bs = bvc * dim * 4 + bvc * 8 + 16
    nb = (n + bvc - 1) // bvc
    blob = bytearray(nb * bs)
    keep = np.zeros(nb, np.uint32)
    for b in range(nb):
        r = rows[b * bvc:(b + 1) * bvc]
        o = b * bs
        blob[o:o + r.nbytes] = r.tobytes()
        kk = keys[b * bvc:(b + 1) * bvc].astype(np.uint64)
        blob[o + bvc * dim * 4:o + bvc * dim * 4 + kk.nbytes] = kk.tobytes()
        keep[b] = (1 << len(r)) - 1 if len(r) < 32 else 0xffffffff
    return bytes(blob), nb, bs, keep


@pytest.mark.parametrize("mutation", ["append", "append_dev", "put", "put_holes", "load_features", "load_blocks", "reserve"])
def test_every_mutation_drops_the_twin(zv, oracle, mutation):
    """after any mutation the twin is gone (a stale one would certify rows that no longer exist: here a far row is overwritten, or
    rows are added, with copies of the queries); the next search is the oracle's on the new rows, and so is one through a new twin"""
    import torch
    from zvec_amd import _lib
    rng = np.random.default_rng(71)
    n, dim, nq, k = 30000, 48, 70, 10
    base, q = _clustered(rng, n, dim, nq, 0.2)
    se = zv.HipFlatStreamer(dim, L2)
    assert se.add_batch(base, np.arange(n, dtype=np.uint64)) == 0
    se.set_shadow(True)
    new = base.copy()
    far = np.argsort(-exact_l2(base[:4000], q).min(0))[:nq]        # rows far from every query
    qcopy = q + np.float32(1e-3)
    L = _lib.lib()
    if mutation == "append":
        assert se.add_batch(qcopy, np.arange(n, n + nq, dtype=np.uint64)) == 0
        new = np.concatenate([base, qcopy])
    elif mutation == "append_dev":
        d = torch.from_numpy(qcopy).cuda()
        torch.cuda.synchronize()
        assert se.add_batch_dev(d.data_ptr(), nq) == 0
        torch.cuda.synchronize()
        new = np.concatenate([base, qcopy])
    elif mutation == "put":
        assert se.add_with_id_batch(far.astype(np.uint32), qcopy) == 0
        new[far] = qcopy
    elif mutation == "put_holes":
        ids = np.arange(n + 40, n + 40 + nq, dtype=np.uint32)            # 40 holes between the old rows and the new ones
        assert se.add_with_id_batch(ids, qcopy) == 0
        new = np.concatenate([base, np.zeros((40, dim), np.float32), qcopy])
    elif mutation == "load_features":
        fk = np.arange(n, n + nq, dtype=np.uint64)
        assert L.zvec_hip_flat_load_features(se._h, qcopy.tobytes(), qcopy.nbytes, nq, 0, 32, fk.ctypes.data) == 0
        new = np.concatenate([base, qcopy])
    elif mutation == "load_blocks":
        blob, nb, bs, keep = _blocks(qcopy, np.arange(n, n + nq))
        assert L.zvec_hip_flat_load_blocks(se._h, blob, len(blob), nb, bs, 32, keep.ctypes.data) == 0
        new = np.concatenate([base, qcopy])
    else:
        assert se.reserve(4 * n) == 0
    assert not se.shadow_info()["enabled"], mutation + " left the twin in place"
    keys = np.arange(len(new), dtype=np.uint64)
    ex = None
    if mutation == "put_holes":
        from oracle.oracle import pack_bits
        hole = np.zeros(len(new), bool)
        hole[n:n + 40] = True
        ex = pack_bits(hole)
    ok, os_, _, oc = oracle.flat_search(new, q, k, keys=keys, exclude_bits=ex, threads=16)
    band = _fp32_band(L2, q, new)
    gk, gs, gc = flat_search(se, q, k)
    _batch_vs_oracle(mutation + ": after", L2, (gk, gs, gc), 1, (ok, os_, oc), band)
    se.set_shadow(True)
    gk, gs, gc, rerun = flat_search_dev(se, q, k)
    _batch_vs_oracle(mutation + ": new twin", L2, (gk, gs, gc), rerun, (ok, os_, oc), band)
