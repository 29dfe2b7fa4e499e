"""Group-by search on HNSW graphs on the GPU (zvec_hip_hnsw_search_grouped[_dev], DESIGN §3c "Group-by") against the fp64 model of
tests/hnsw_group_ref.py on its fixtures.  All data is exact (small integers: fp32 equals fp64), so every comparison is for equality:
groups, keys, score bits, counts, out_ngroups, distances computed and nodes expanded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_group_ref as G  # noqa: E402
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

NOKEY, FLT_MAX = 0xffffffffffffffff, 3.4028234663852886e38
CASES = G.cases()


def _loaded(g, metric="l2", dtype="fp32"):
    import zvec_amd as zv
    se = zv.HipHnswSearcher(g.rows.shape[1], {"l2": "SquaredEuclidean", "ip": "InnerProduct"}[metric], dtype=dtype)
    up = [g.upper_of, g.nbr_up, g.cnt_up] if g.max_level > 0 else [None] * 3
    assert se.load(g.rows, g.nbr0, g.cnt0, g.entry_point, g.keys, *up) == 0
    return se


def _outputs(count, gnum, gk, fill=0):
    """groups, ngroups, keys, scores, counts"""
    return [np.full(s, fill, t) for s, t in (((count, gnum), np.uint32), (count, np.uint32), ((count, gnum, gk), np.uint64),
                                             ((count, gnum, gk), np.float32), ((count, gnum), np.uint32))]


def _call(se, ctx, c, out):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    q = np.ascontiguousarray(c.q, se.np_dtype)
    ex = None if c.exclude is None else H.words_of(c.exclude)
    return _lib.lib().zvec_hip_hnsw_search_grouped(se._h, ctx._h, _np_ptr(q), q.shape[0], _np_ptr(c.group_of), c.ngroups, c.group_num,
                                                   c.group_topk, c.ef, c.max_scan, FLT_MAX if c.threshold is None else c.threshold,
                                                   _np_ptr(ex), *[_np_ptr(o) for o in out])


def _search(se, c):
    """the five outputs, then scanned, hops and the slices of the batch"""
    ctx = se.create_context()
    out = _outputs(c.q.shape[0], c.group_num, c.group_topk, 7)
    assert _call(se, ctx, c, out) == 0
    return out + list(se.last_stats(ctx, c.q.shape[0]))


def _equals_model(res, ms, c):
    groups, ngroups, keys, scores, counts, scanned, hops, _ = res
    for i, m in enumerate(ms):
        ng = len(m.groups)
        assert ngroups[i] == ng and groups[i].tolist() == m.groups + [G.NONE] * (c.group_num - ng), i
        assert counts[i].tolist() == m.counts + [0] * (c.group_num - ng) and (scanned[i], hops[i]) == (m.scanned, m.hops), i
        want_k = np.full((c.group_num, c.group_topk), NOKEY, np.uint64)
        want_s = np.full((c.group_num, c.group_topk), np.inf, np.float32)
        for j in range(ng):
            want_k[j, :len(m.keys[j])], want_s[j, :len(m.keys[j])] = m.keys[j], m.scores[j]
        assert keys[i].tobytes() == want_k.tobytes() and scores[i].tobytes() == want_s.tobytes(), i


@pytest.fixture(scope="module")
def models():
    return {name: G.model_of(c) for name, c in CASES.items()}


@pytest.mark.parametrize("name,dtype", [(name, "fp32") for name in CASES] + [("7x4_ef9", "fp16"), ("chain_insert_in_front", "fp16")])
def test_equals_model(name, dtype, models):
    """fp16: the rows are binary16 values, and both handles equal the model bit for bit, so they equal each other"""
    c, ms = CASES[name], models[name]
    assert c.fact(ms) and (c.g.rows.astype(np.float16) == c.g.rows).all()
    _equals_model(_search(_loaded(c.g, c.metric, dtype), c), ms, c)


def test_sliced_and_device_pointers(models):
    """40 queries under the smallest workspace go in at least 3 slices; the device-pointer entry answers as the host entry"""
    import torch
    from zvec_amd import _lib
    c, ms = CASES["7x4_ef60"], models["7x4_ef60"]
    se, count = _loaded(c.g), c.q.shape[0]
    _lib.check(_lib.lib().zvec_hip_set_option(b"hnsw_ws_bytes", 1024), "set_option")
    try:
        res = _search(se, c)
    finally:
        _lib.check(_lib.lib().zvec_hip_set_option(b"hnsw_ws_bytes", 1 << 30), "set_option")
    assert res[7] >= 3
    _equals_model(res, ms, c)
    signed = lambda x: x.view(np.int32 if x.itemsize == 4 else np.int64)       # (the bytes travel; torch has no unsigned types for them)
    dev = [torch.from_numpy(signed(x)).cuda() for x in [c.q, c.group_of] + _outputs(count, c.group_num, c.group_topk)]
    ctx = se.create_context()
    assert se.search_grouped_dev(dev[0].data_ptr(), count, dev[1].data_ptr(), c.ngroups, c.group_num, c.group_topk, c.ef, c.max_scan,
                                 *[d.data_ptr() for d in dev[2:]], ctx) == 0
    stats = se.last_stats(ctx, count)                # (waits for the context's stream)
    assert [d.cpu().numpy().tobytes() for d in dev[2:]] == [x.tobytes() for x in res[:5]]
    assert [s.tolist() for s in stats[:2]] == [res[5].tolist(), res[6].tolist()] and stats[2] == 1


def test_refusals_and_empty_index():
    c = CASES["chain_groups"]
    se = _loaded(c.g)
    for code, over in ((-31, dict(group_num=0)), (-31, dict(group_topk=0)), (-31, dict(group_of=None)), (-12, dict(group_num=27, group_topk=19)),
                       (-12, dict(ef=513))):
        out = _outputs(1, 27, 19, 7)
        assert _call(se, se.create_context(), c._replace(**over), out) == code and all((o == 7).all() for o in out), over
    empty = c._replace(g=H.graph_of(np.zeros((0, 4), np.float32), []), group_of=None)
    res = _search(_loaded(empty.g), empty)
    _equals_model(res, G.model_of(empty), empty)
    assert res[1].tolist() == [0]


def test_python_group_by_search_impl(models):
    c, ms = CASES["3x2_ef40"], models["3x2_ef40"]
    se = _loaded(c.g)
    ctx = se.create_context()
    ctx.set_group_params(c.group_num, c.group_topk)
    ctx.set_group_by(lambda key: "g%d" % (((key - 3) // 7) % 7))     # (exact_graph: key = 7 * node + 3)
    assert se.group_by_search_impl(c.q, c.q.shape[0], ctx, c.ef) == 0
    for i, m in enumerate(ms):
        got = ctx.group_result(i)
        assert [x.group_id() for x in got] == ["g%d" % k for k in m.groups]
        assert [[(d.key(), d.score()) for d in x.docs()] for x in got] == [list(zip(k.tolist(), s.tolist())) for k, s in zip(m.keys, m.scores)]
