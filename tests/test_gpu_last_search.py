"""What a search leaves on its context belongs to the LAST user-facing search of that context (zvec_amd/csrc/host/last_search.h,
DESIGN §3 "What a search leaves on its context"): one context, one small index of every family, and after a search of family B every
reader of family A has nothing to report — zvec_hip_ctx_last_route 0, zvec_hip_ctx_last_ivf_plan ROUTE_NONE, every reader that takes a
handle NoReady (-21) — until A searches again, when it reports what it reported before.  Then the named cases: the plan buffer
outgrown by a by-positions search between an IVF search and its statistics, two handles of one family on a shared context, and a
certify step that an HNSW search in between has dropped."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_READY, INVALID = -21, -31
N, DIM, NLIST, NQ, TOPK, NODES = 256, 16, 4, 4, 3, 64
NPROBE, REFINE, EF = 2, 4, 16


def _runs(dense):
    nz = dense != 0
    return nz.sum(1).astype(np.uint32), np.nonzero(nz)[1].astype(np.uint32), dense[nz]


class Family:
    """one index, its search on a context and its reader: read(ctx) -> (rc, values); rc None = the family has no reader"""

    def __init__(self, name, se, search, read):
        self.name, self.se, self.search, self.read = name, se, search, read


def _read_handle(fn, se, ctx, shapes, *extra):
    """a reader that takes a handle: (rc, the arrays it filled)"""
    out = [np.zeros(s, t) for s, t in shapes]
    rc = fn(se._h, ctx._h, NQ, *extra, *[C.c_void_p(a.ctypes.data) for a in out])
    return rc, tuple(a.tobytes() for a in out)


def _ivf_read(se, ctx):
    import zvec_amd._lib as L
    rc, vals = _read_handle(L.lib().zvec_hip_ivf_last_stats, se, ctx, [(NQ, np.uint32)] * 2)
    route = ctx.last_ivf_plan()["route"]
    assert (route == L.IVF_ROUTE_NONE) == (rc == NO_READY)        # both IVF readers follow the same record
    return rc, vals + (route,)


def _bivf_read(se, ctx):
    import zvec_amd._lib as L
    kc = TOPK * REFINE
    rc, probes = _read_handle(L.lib().zvec_hip_bivf_last_probes, se, ctx, [((NQ, NPROBE), np.uint32), (NQ, np.uint32), (NQ, np.uint32)])
    rc2, cands = _read_handle(L.lib().zvec_hip_bivf_last_candidates, se, ctx,
                              [((NQ, kc), np.uint32), ((NQ, kc), np.float32), (NQ, np.uint32)], kc)
    assert rc == rc2                                              # the fp32 search leaves both readable, any other search neither
    return rc, probes + cands


def _hnsw_read(fn_name):
    def read(se, ctx):
        import zvec_amd._lib as L
        slices = C.c_uint32(0)
        scanned, hops = np.zeros(NQ, np.uint32), np.zeros(NQ, np.uint32)
        rc = getattr(L.lib(), fn_name)(se._h, ctx._h, NQ, C.c_void_p(scanned.ctypes.data), C.c_void_p(hops.ctypes.data), C.byref(slices))
        return rc, (scanned.tobytes(), hops.tobytes(), int(slices.value))
    return read


def _ivf(rows, seed):
    import zvec_amd as zv
    from tests.util import kmeans_lists
    cent, offs, order = kmeans_lists(np.random.default_rng(seed), rows, NLIST)
    se = zv.HipIVFSearcher(DIM, "SquaredEuclidean", scan_ratio=NPROBE / NLIST, brute_force_threshold=10)
    assert se.load(cent, offs, rows[order], order.astype(np.uint64)) == 0
    return se


def _hnsw(rows):
    import zvec_amd as zv
    se = zv.HipHnswSearcher(DIM)
    assert se.build(rows, m=8, m0=16, ef_construction=16) == 0
    return se


@pytest.fixture(scope="module")
def world():
    """the shared context, the queries and one index of every family (integer data: every search is repeatable bit for bit)"""
    import zvec_amd as zv
    rng = np.random.default_rng(20261126)
    rows = rng.integers(-8, 9, (N, DIM)).astype(np.float32)
    rows[rows == 0] = 1
    q = rng.integers(-8, 9, (NQ, DIM)).astype(np.float32)
    q[q == 0] = 1
    flat = zv.HipFlatSearcher(DIM, "SquaredEuclidean")
    assert flat.load(rows) == 0
    ivf = _ivf(rows, 1)
    bivf = zv.HipHammingIVFSearcher(32)
    assert bivf.build_fp32(rows, NLIST, "SquaredEuclidean", kmeans_iters=3, seed=5) == 0
    hnsw = _hnsw(rows[:NODES])
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = hnsw.export()        # the same graph over the same rows, held as sparse runs
    shnsw = zv.HipHnswSparseSearcher()
    assert shnsw.load(*_runs(rows[:NODES]), nbr0, cnt0, hnsw.info()["entry_point"], keys, upper_of, nbr_up, cnt_up) == 0
    sparse = zv.HipFlatSparseStreamer()
    assert sparse.add_batch(*_runs(rows)) == 0
    ctx = zv.IndexContext()
    ctx.set_topk(TOPK)
    fams = [
        Family("flat", flat, lambda c: flat.search_impl(q, NQ, c), lambda se, c: (0 if c.last_route() else NO_READY, (c.last_route(),))),
        Family("ivf", ivf, lambda c: ivf.search_impl(q, NQ, c), _ivf_read),
        Family("hamming ivf", bivf, lambda c: bivf.search_impl_fp32(q, NQ, c, refine=REFINE, nprobe=NPROBE, max_scan=N), _bivf_read),
        Family("hnsw", hnsw, lambda c: hnsw.search(q, NQ, c, EF), _hnsw_read("zvec_hip_hnsw_last_stats")),
        Family("sparse hnsw", shnsw, lambda c: shnsw.search(*_runs(q), NQ, c, EF), _hnsw_read("zvec_hip_hnsw_sparse_last_stats")),
        Family("sparse flat", sparse, lambda c: sparse.search_impl(*_runs(q), NQ, c), lambda se, c: (None, ())),
    ]
    return dict(ctx=ctx, rows=rows, q=q, fams={f.name: f for f in fams})


def _gone(f, ctx, what):
    rc, vals = f.read(f.se, ctx)
    assert rc in (None, NO_READY), "%s: %s still reports rc %r" % (what, f.name, rc)
    if f.name == "flat":
        assert ctx.last_route() == 0, what


def _there(f, ctx, what):
    rc, vals = f.read(f.se, ctx)
    assert rc in (None, 0), "%s: %s reports rc %r" % (what, f.name, rc)
    return vals


def test_fresh_context_has_nothing_to_report(world):
    import zvec_amd as zv
    ctx = zv.IndexContext()
    for f in world["fams"].values():
        _gone(f, ctx, "fresh context")


@pytest.mark.parametrize("a,b", list(itertools.permutations(["flat", "ivf", "hamming ivf", "hnsw", "sparse hnsw", "sparse flat"], 2)))
def test_readers_follow_the_last_search(world, a, b):
    ctx, A, B = world["ctx"], world["fams"][a], world["fams"][b]
    what = "%s then %s" % (a, b)
    assert A.search(ctx) == 0
    kept = _there(A, ctx, what + ": after the first search")
    assert B.search(ctx) == 0
    _gone(A, ctx, what)
    _there(B, ctx, what)
    assert A.search(ctx) == 0
    assert _there(A, ctx, what + ": searched again") == kept, what
    _gone(B, ctx, what + ": searched again")


@pytest.mark.parametrize("nq", [NQ, 16])                  # the direct route (q_nprobe | q_scanned head the plan) and the tile route
def test_ivf_statistics_after_the_plan_buffer_was_outgrown(world, nq):
    """An IVF search, then a flat by-positions search of 4 x 1000 positions = 16 KB of plan, far beyond the IVF plan's (direct route:
    3 x nq + 8 words; tile route at nlist 4: a few hundred words) and the 25 % + 256 bytes the buffer grows by: the buffer is
    reallocated.  The statistics of the IVF search are gone (they were read through pointers into the freed block once), and come
    back equal, through the offsets, when the index searches again in the moved buffer."""
    import zvec_amd as zv
    import zvec_amd._lib as L
    ivf, flat = world["fams"]["ivf"].se, world["fams"]["flat"].se
    q = np.resize(world["q"], (nq, DIM))
    ctx = zv.IndexContext()
    ctx.set_topk(TOPK)
    assert ivf.search_impl(q, nq, ctx) == 0
    want = (L.IVF_ROUTE_TILE,) if nq > 8 else (L.IVF_ROUTE_DIRECT_BLOCK_TOPK, L.IVF_ROUTE_DIRECT_SELECT)
    assert ctx.last_ivf_plan()["route"] in want
    scanned, probes = ivf.last_stats(ctx, nq)
    assert (probes >= 1).all() and (probes <= NPROBE).all() and (scanned > 0).all() and (scanned <= N).all()
    with pytest.raises(L.ZvecHipError) as e:
        ivf.last_stats(ctx, nq + 1)
    assert e.value.code == NO_READY
    positions = [np.arange(1000) % N] * NQ
    assert flat.search_by_positions_impl(world["q"], positions, NQ, ctx) == 0
    with pytest.raises(L.ZvecHipError) as e:
        ivf.last_stats(ctx, nq)
    assert e.value.code == NO_READY and ctx.last_ivf_plan()["route"] == L.IVF_ROUTE_NONE
    assert ivf.search_impl(q, nq, ctx) == 0
    again = ivf.last_stats(ctx, nq)
    assert np.array_equal(again[0], scanned) and np.array_equal(again[1], probes)


def test_two_ivf_indexes_on_one_context(world):
    A, ctx = world["fams"]["ivf"], world["ctx"]
    other = _ivf(world["rows"][::-1].copy(), 2)
    assert A.search(ctx) == 0
    assert _ivf_read(A.se, ctx)[0] == 0 and _ivf_read_handle_only(other, ctx) == NO_READY
    assert other.search_impl(world["q"], NQ, ctx) == 0
    assert _ivf_read_handle_only(A.se, ctx) == NO_READY and _ivf_read_handle_only(other, ctx) == 0


def _ivf_read_handle_only(se, ctx):
    import zvec_amd._lib as L
    return _read_handle(L.lib().zvec_hip_ivf_last_stats, se, ctx, [(NQ, np.uint32)] * 2)[0]


def test_two_hnsw_graphs_on_one_context(world):
    A, ctx = world["fams"]["hnsw"], world["ctx"]
    other = _hnsw(world["rows"][NODES:2 * NODES])
    read = A.read
    assert A.search(ctx) == 0
    assert read(A.se, ctx)[0] == 0 and read(other, ctx)[0] == NO_READY
    assert other.search(world["q"], NQ, ctx, EF) == 0
    assert read(A.se, ctx)[0] == NO_READY and read(other, ctx)[0] == 0


def test_certify_step_is_dropped_by_a_search_in_between(world):
    """A flat search through the fp16 twin leaves a certify step pending: asking for it with another batch size is refused, which
    shows that it is there.  After an HNSW search on the same context nothing is pending: the same call returns 0, nothing re-run —
    what it does after a flat search that did not go through the twin."""
    import torch
    import zvec_amd as zv
    import zvec_amd._lib as L
    from tests.util import dev_lists
    hnsw, ctx, q = world["fams"]["hnsw"], world["ctx"], world["q"]
    tw = zv.HipFlatSearcher(DIM, "SquaredEuclidean")
    assert tw.load(world["rows"]) == 0
    tw.set_shadow(True)
    assert tw.shadow_width(TOPK) > TOPK
    dq, keys, scores, counts, _ = dev_lists(q, TOPK, None)
    torch.cuda.synchronize()
    args = (keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx)
    assert tw.search_dev(dq.data_ptr(), NQ, TOPK, *args) == 0
    with pytest.raises(L.ZvecHipError) as e:
        tw.shadow_certify(dq.data_ptr(), NQ - 1, TOPK, *args)
    assert e.value.code == INVALID
    assert hnsw.search(ctx) == 0
    assert tw.shadow_certify(dq.data_ptr(), NQ - 1, TOPK, *args) == 0
    assert tw.shadow_certify(dq.data_ptr(), NQ, TOPK, *args) == 0
    torch.cuda.synchronize()
    # ... and the step of a search that nothing came after is still served
    assert tw.search_dev(dq.data_ptr(), NQ, TOPK, *args) == 0
    assert tw.shadow_certify(dq.data_ptr(), NQ, TOPK, *args) in range(NQ + 1)
    torch.cuda.synchronize()
