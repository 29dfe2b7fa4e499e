"""The fixtures of tests/test_gpu_ivf_routes.py held to what they are there for, without a GPU (tests/ivf_routes_ref.py).

For every cell — route x metric x element type x dim x data kind — the route rule gives the route the cell is named after, and the
reference made wrong in one way at a time (the scan's last k-step dropped, probe_cnt ignored, the probe lists sorted by id, the
exclusion ignored, the radius ignored, the inner-product radius with the wrong sign) answers differently for at least one query of
the cell: a kernel with that mistake fails the GPU test.  Exact kinds tie at the k-th place, gaussian kinds leave most k-th places
decided beyond the select band, every radius keeps its distance from every score."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_plan_ref as P  # noqa: E402
import ivf_routes_ref as R  # noqa: E402

INDEXES = [(m, t, d, kind) for m in R.METRICS for t in R.DTYPES for d in R.DIMS[t] for kind in R.kinds_of(m)]


def test_dims_stand_around_the_k_step():
    for t in R.DTYPES:
        ks = R.KSTEP[t]
        assert ks * np.dtype(R.NP_DTYPE[t]).itemsize == 128
        below, at, above, several = R.DIMS[t]
        assert below < ks == at < above < 2 * ks and several > 3 * ks and several % ks
        assert [R.last_kstep(t, d) for d in R.DIMS[t]] == [0, 0, ks, several // ks * ks]
    t, d = R.RAW_ROWS
    # api_ivf_core.inc.h: dim_in == dscan (no norm slot), dpad x 4 == row_bytes (fp32: the dim is whole k-steps)
    assert d in R.DIMS[t] and t == "fp32" and d % R.KSTEP[t] == 0


def test_list_sizes_and_routes():
    sz = R.SIZES
    assert sz.size == 24 and {0, 1, 127, 128, 129} <= set(sz.tolist()) and 2500 <= sz.sum() <= 3500
    assert sorted(sz[list(R.LARGE)].tolist()) == sorted(sz[sz >= 400].tolist()) and ((sz[sz >= 400] <= 700).all())
    assert R.runs_of(2) == 1 and R.runs_of(5) == 2
    seen = set()
    for name, (route, nprobe, batches) in R.ROUTES.items():
        for nq, k in batches:
            assert P.expected_route(nq, k, nprobe, sz) == route, (name, nq, k)
            seen.add((route, R.runs_of(nprobe) if route == P.ROUTE_DIRECT_SELECT else 0))
        assert sorted(b[0] for b in batches) == ([1, 8] if name in R.DIRECT else [9, 40])
        assert max(b[1] for b in batches) <= 500 and (route != P.ROUTE_LARGE_K or min(b[1] for b in batches) > P.FUSED_MAX_K)
    assert seen == {(P.ROUTE_DIRECT_BLOCK_TOPK, 0), (P.ROUTE_DIRECT_SELECT, 1), (P.ROUTE_DIRECT_SELECT, 2), (P.ROUTE_TILE, 0),
                    (P.ROUTE_LARGE_K, 0)}


@pytest.mark.parametrize("nq,nprobe", [(b[0], v[1]) for v in R.ROUTES.values() for b in v[2]])
def test_probe_lists(nq, nprobe):
    ids, cnt = R.probe_lists(nq, nprobe, 31)
    assert ids.shape == (nq, nprobe) and cnt.min() >= 1 and cnt.max() == nprobe
    assert nq < nprobe or set(cnt.tolist()) == set(range(1, nprobe + 1))
    for q in range(nq):
        assert len(set(ids[q].tolist())) == nprobe and set(ids[q, :cnt[q]].tolist()) & set(R.LARGE)
    assert nq == 1 or any((np.diff(ids[q]) < 0).any() for q in range(nq))        # in no order


def _changes(ix, c, args, wrong):
    return not R.same(R.answer(ix, c["q"], c["ids"], c["cnt"], c["k"], **args), R.answer(ix, c["q"], c["ids"], c["cnt"], c["k"], wrong=wrong, **args))


@pytest.mark.parametrize("metric,dtype,d,kind", INDEXES)
def test_every_cell_discriminates(metric, dtype, d, kind):
    ix = R.index(metric, dtype, d, kind)
    assert ix["vecs"].dtype == R.NP_DTYPE[dtype] and ix["dim"] == d + (R.NORM_SLOTS[dtype] if metric == R.COS else 0)
    if kind == "exact":                                          # exact in either format: integers, sums below 2^11
        assert (ix["vecs"] == np.round(ix["vecs"])).all() and d * 7 * 7 < 2 ** 24 and ix["vecs"].max() < 2 ** 11
    in_list = across = False
    for route in R.ROUTES:
        tied = decided = total = short = full = cut = 0
        changed = dict.fromkeys(R.WRONG, False)
        for batch in (0, 1):
            c = R.case(ix, route, batch)
            nq, k, v, plain = c["nq"], c["k"], c["variants"], c["plain"]
            what = "%s %s batch %d" % (ix["name"], route, nq)
            total += nq
            # the mistakes, each against the variant that shows it
            for wrong, variant in (("last_kstep", "plain"), ("probe_cnt", "plain"), ("sorted_lists", "plain"), ("exclusion", "exclusion"),
                                   ("radius", "radius"), ("radius_sign", "radius")):
                if wrong == "radius_sign" and metric != R.IP:
                    continue
                changed[wrong] |= _changes(ix, c, v[variant], wrong)
            # the exclusion takes a whole probed list out
            assert c["whole"] in c["ids"][0, :c["cnt"][0]] and c["whole"] in R.LARGE
            ex = v["exclusion"]["excluded"]
            offs = P.list_offsets(R.SIZES)
            assert ex[offs[c["whole"]]:offs[c["whole"] + 1]].all() and 0.2 < ex.mean() < 0.6
            # the radius: clear of every score of every counted row, some lists cut and not all
            r = v["radius"]["radius"]
            band = 0.0 if kind == "exact" else float(R.select_band(ix, c["q"])[1].max())
            dist = min(float(np.abs(s - r).min()) for s in R.all_scores(ix, c["q"], c["ids"], c["cnt"]))
            assert dist > band and dist > 0, "%s: radius %r within %r of a score (band %r)" % (what, r, dist, band)
            cut_r = R.answer(ix, c["q"], c["ids"], c["cnt"], k, radius=r)
            assert (cut_r["counts"] <= plain["counts"]).all()
            short += int((cut_r["counts"] < plain["counts"]).sum())
            full += int((cut_r["counts"] == plain["counts"]).sum())
            assert (cut_r["counts"] > 0).any(), what
            far = R.answer(ix, c["q"], c["ids"], c["cnt"], k, radius=v["radius_far"]["radius"])
            assert R.same(far, plain) and v["radius_far"]["radius"] > max(float(s.max()) for s in R.all_scores(ix, c["q"], c["ids"], c["cnt"]))
            # the scan limit
            ms = R.answer(ix, c["q"], c["ids"], c["cnt"], k, max_scan=v["max_scan"]["max_scan"])
            cut += sum(len(ms["probed"][i]) < int(c["cnt"][i]) for i in range(nq))
            # the k-th place
            if kind == "exact":
                for i in range(nq):
                    if plain["gap"][i] == 0:
                        tied += 1
                        s = plain["cand"][i]
                        # the rows that tie with the k-th: where do they lie?
                        full_ref = R.answer(ix, c["q"][i:i + 1], c["ids"][i:i + 1], c["cnt"][i:i + 1], len(s))
                        rows = full_ref["pos"][0][full_ref["scores"][0] == s[k - 1]]
                        lists = np.searchsorted(offs, rows, side="right") - 1
                        in_list |= np.bincount(lists).max() > 1
                        across |= np.unique(lists).size > 1
            else:
                decided += int((plain["gap"] > 2.0 * R.select_band(ix, c["q"])[1]).sum())
        assert all(changed[w] for w in R.WRONG if w != "radius_sign" or metric == R.IP), "%s %s: unchanged under %r" % (
            ix["name"], route, [w for w in R.WRONG if not changed[w]])
        assert short > 0 and full > 0, "%s %s: the radius cuts %d lists and leaves %d" % (ix["name"], route, short, full)
        assert cut > 0, "%s %s: the scan limit cuts nothing" % (ix["name"], route)
        if kind == "exact":
            assert tied * 4 >= total, "%s %s: %d of %d queries tie at the k-th place" % (ix["name"], route, tied, total)
        else:
            assert decided * 4 >= total * 3, "%s %s: %d of %d k-th places decided beyond the band" % (ix["name"], route, decided, total)
    if kind == "exact":
        assert in_list and across, "%s: ties inside one list %r, across lists %r" % (ix["name"], in_list, across)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("nlist,step,margin", [(R.COARSE_NLIST, R.COARSE_STEP, 0.01), (R.NLIST, 0.125, 0.002)])
def test_coarse_fixtures_are_untied(metric, dtype, nlist, step, margin):
    """the ranking of ALL lists is decided by a margin far above binary16 rounding (2^-11 relative: the cosine scores are at most 2,
    the margin of the 12-list fixture ten times 2^-10; the L2 and inner-product scores are exact integers or quarters a unit apart);
    the 24-list fixture only has to rank alike in two fp32 kernels"""
    for nq in (1, 8, 9, 40):
        cent, q, d = R.coarse_fixture(metric, dtype, nq, nlist=nlist, step=step)
        assert cent.dtype == q.dtype == R.NP_DTYPE[dtype] and cent.shape[1] == q.shape[1] == d + (R.NORM_SLOTS[dtype] if metric == R.COS else 0)
        order, s = R.coarse_ranking(metric, cent, q, d)
        assert np.diff(s, axis=1).min() >= (margin if metric == R.COS else 1.0), np.diff(s, axis=1).min()
        assert margin >= 4 * 2.0 ** -11
        assert all(sorted(order[i].tolist()) == list(range(nlist)) for i in range(nq))
