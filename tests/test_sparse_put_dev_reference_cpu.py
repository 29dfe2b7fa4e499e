"""The cases of tests/test_gpu_sparse_put_dev.py held to what they claim, against the Python model alone (no GPU, no library): every
step takes the route it names, the splice case crosses the chunk boundaries it says it crosses for whatever chunk size it is given,
both parities reach the stage gather and the splice, and the keep-last case names an id three times, descending."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_put_dev_ref as G  # noqa: E402
import sparse_put_ref as M  # noqa: E402

DTYPES = ["fp32", "fp16"]
CHUNKS = [4096, 1024, 8192, 1000]


def _walk(steps, dtype):
    """(step, its plan on the model in front of it, the model in front of it) for every step; the claimed routes are checked"""
    model = M.PutModel(dtype)
    out = []
    for step in steps:
        if step["kind"] == "put":
            p = G.plan(model, step)
            assert p["route"] == step["route"], (step["ids"], p["route"], step["route"])
            out.append((step, p, model.copy()))
        G.apply_step(model, step)
    return out, model


def _all_cases(dtype, chunk):
    cases = {"tail": G.case_tail(dtype), "in place": G.case_in_place(dtype), "splice": G.case_splice(dtype, chunk)[0],
             "keep last": G.case_keep_last(dtype)}
    for off in (1, 2, 3):
        cases["alignment %d" % off] = G.case_alignment(dtype, off)
    for metric in ("InnerProductSparse", "SquaredEuclideanSparse"):
        cases["search " + metric] = G.case_search(dtype, metric)[0]
    return cases


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_step_takes_the_route_it_claims(dtype):
    routes = set()
    for name, steps in _all_cases(dtype, CHUNKS[0]).items():
        walked, _ = _walk(steps, dtype)
        routes |= {p["route"] for _, p, _ in walked}
        for step, _, _ in walked:                      # a call the library would refuse is no case: at most 4096 ascending pairs a row
            for idx, val in step["rows"]:
                assert idx.size == val.size <= 4096 and np.all(np.diff(idx.astype(np.int64)) > 0), name
    assert routes == {0, 1, 2}


@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_case_makes_holes_fills_one_and_is_appended_to(dtype):
    steps = G.case_tail(dtype)
    walked, model = _walk(steps, dtype)
    first = walked[0][2]
    assert first.count() == 0 and walked[0][1]["route"] == 0
    holes_after_two = walked[2][2].holes
    assert len(holes_after_two) >= 3
    assert steps[2]["ids"][0] in holes_after_two and steps[3]["ids"][0] in holes_after_two          # puts into holes
    assert len(steps[2]["rows"][0][0]) > 0 and len(steps[3]["rows"][0][0]) == 0
    assert steps[4]["kind"] == "append" and walked[4][2].holes and walked[4][2].count() > 64       # a second word of hole bits
    assert len(model.holes) > len(walked[4][2].holes)                                              # and a gap behind the appended rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_case_holds_an_empty_and_a_full_row(dtype):
    walked, _ = _walk(G.case_in_place(dtype), dtype)
    lens = {len(r[0]) for r in walked[1][0]["rows"]}
    assert 0 in lens and 4096 in lens and walked[1][1]["route"] == 1 and walked[2][1]["route"] == 1
    assert any(i >= walked[2][2].count() for i in walked[2][0]["ids"])


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_splice_case_sits_on_the_chunk_boundaries(dtype, chunk):
    steps, (a, b, c) = G.case_splice(dtype, chunk)
    walked, _ = _walk(steps, dtype)
    store = walked[1][2]                                # the store the first splice meets
    off = G.offsets(store)
    assert 3 * chunk < store.elements() <= 3 * chunk + 100
    assert off[a + 1] == chunk and off[b + 1] == 2 * chunk - 1 and off[c + 1] == 3 * chunk + 1
    step, p, _ = walked[1]
    assert step["ids"] == [a, b, c] and p["route"] == 2
    for i, r in zip(step["ids"], step["rows"]):
        assert abs(len(r[0]) - store.rows[i][0].size) == 1          # one longer or one shorter
    shifts = [s for _, p, _ in walked[1:] for s in p["shifts"]]
    assert {s & 1 for s in shifts} == {0, 1} and all(p["route"] == 2 for _, p, _ in walked[1:])
    assert walked[2][1]["descending"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_parities_reach_the_stage(dtype):
    for off in (1, 2, 3):
        steps = G.case_alignment(dtype, off)
        walked, _ = _walk(steps, dtype)
        assert [len(r[0]) for r in steps[0]["rows"]] == [1, 2, 3, 63, 64, 65, 257]
        for step, p, _ in walked[:2]:                   # in call order the view's offset alone decides
            assert step["src_off"] == off and set(p["stage_parities"]) == {off & 1}
        assert [p["route"] for _, p, _ in walked] == [0, 1, 2] and walked[2][1]["descending"]
    # every kept row with pairs begins at an even or an odd place of the stage: both occur (the head and tail halves)
    sb = np.concatenate([[0], np.cumsum(G.ALIGN_LENGTHS)])
    assert {int(x) & 1 for x in sb[:-1]} == {0, 1} and {int(x) & 1 for x in sb[1:]} == {0, 1}
    # without an offset: the descending splice step and the keep-last case still reach both
    par = {q for _, p, _ in _walk(G.case_splice(dtype, CHUNKS[0])[0], dtype)[0] for q in p["stage_parities"]}
    assert par == {0, 1}
    par = {q for _, p, _ in _walk(G.case_keep_last(dtype), dtype)[0] for q in p["stage_parities"]}
    assert par == {0, 1}


@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_last_case_names_an_id_three_times_descending(dtype):
    steps = G.case_keep_last(dtype)
    walked, model = _walk(steps, dtype)
    assert sorted(p["route"] for _, p, _ in walked[1:]) == [0, 1, 2]
    for step, p, before in walked[1:]:
        ids = step["ids"]
        thrice = [d for d in set(ids) if ids.count(d) == 3]
        assert len(thrice) == 1 and p["descending"] and len(p["dropped"]) == 2
        named = [i for i, d in enumerate(ids) if d == thrice[0]]
        assert len({len(step["rows"][i][0]) for i in named}) == 3                 # rows of different lengths
        assert p["keep"] != sorted(p["keep"])                                     # the plan's order is not the call's
        after = before.copy()
        G.apply_step(after, step)
        kept = step["rows"][named[-1]]
        assert np.array_equal(after.rows[thrice[0]][0], kept[0]) and M.raw(after.rows[thrice[0]][1]).tobytes() == M.raw(kept[1]).tobytes()
        if step["keys"] is not None:
            assert after.keys[thrice[0]] == step["keys"][named[-1]]


@pytest.mark.parametrize("metric", ["InnerProductSparse", "SquaredEuclideanSparse"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_case_mixes_the_routes_and_leaves_holes(dtype, metric):
    steps, queries = G.case_search(dtype, metric)
    walked, model = _walk(steps, dtype)
    assert {p["route"] for _, p, _ in walked} == {0, 1, 2}
    assert len(model.holes) > 20 and len(queries[0]) == 9 and queries[2].dtype == M.NP[dtype]
    assert any(p["dropped"] for _, p, _ in walked)
