"""Sparse fp32 rows under InnerProductSparse on the GPU (flat index), against tests/sparse_ref.py: every list is checked against
the fp64 reference within the derived band B = (m + 1) * 2^-23 * A; only rows whose bands overlap at the k-th place (or at the
threshold), and the order of equal scores, are left free (check_sparse_lists)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID, NO_EXIST = -12, -31, -22


def _index(rows, keys=None, pieces=None):
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer()
    counts, idx, val = rows
    off = R.offsets(counts)
    cuts = [0, len(counts)] if pieces is None else pieces
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], None if keys is None else keys[a:b]) == 0
    return se


def _search(se, queries, k, threshold=None, exclude=None, ctx=None):
    ctx = ctx or se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


@pytest.mark.parametrize("n,nq,vocab,k,long_queries", R.CASES)
def test_against_the_reference(n, nq, vocab, k, long_queries):
    rows, queries, ref, A, m = R.make_case(n, nq, vocab, long_queries)
    k = n + 5 if k == "n+5" else k
    se = _index(rows)
    assert se.count() == n and se.element_count() == int(rows[0].astype(np.int64).sum())
    keys, scores, counts = _search(se, queries, k)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


def test_keys_given_and_appends_of_unequal_size():
    n, nq = 1000, 65
    rows, queries, ref, A, m = R.make_case(n, nq, 100000, True)
    key_of_row = (np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1 << 40))
    se = _index(rows, keys=key_of_row, pieces=[0, 1, 64, 129, 700, 1000])
    assert se.count() == n
    keys, scores, counts = _search(se, queries, 10)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, 10, None, np.ones(n, bool), key_of_row)


@pytest.mark.parametrize("k", [10, 200])
def test_threshold(k):
    n, nq = 1000, 64
    rows, queries, ref, A, m = R.make_case(n, nq, 50, False)
    se = _index(rows)
    for thr in (-0.75, 0.0, 0.3):
        keys, scores, counts = _search(se, queries, k, threshold=thr)
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, thr, np.ones(n, bool), np.arange(n, dtype=np.uint64))
    assert int(counts.max()) == k


@pytest.mark.parametrize("k", [10, 200])
def test_exclude_bitset_across_chunk_boundaries(k):
    n, nq = 5000, 65
    rows, queries, ref, A, m = R.make_case(n, nq, 50, False)
    se = _index(rows)
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.5
    mask[0:130] = True            # whole chunks of rows, and runs that straddle every chunk boundary near them
    mask[2499:2503] = True
    mask[-1] = True
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(mask))
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, ~mask, np.arange(n, dtype=np.uint64))
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(np.ones(n, bool)))
    assert not counts.any()


def test_empty_index():
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer()
    _, queries, _, _, _ = R.make_case(63, 64, 50, False)
    keys, scores, counts = _search(se, queries, 10)
    assert se.count() == 0 and not counts.any()
    assert se.get_vector_by_id(0) is None


def test_get_vector_round_trip():
    n = 1000
    rows, _, _, _, _ = R.make_case(n, 65, 100000, True)
    se = _index(rows, pieces=[0, 3, 500, 1000])
    counts, idx, val = rows
    off = R.offsets(counts)
    seen = set()
    for pos in list(range(0, 40)) + [97, 499, 500, 501, n - 1]:
        gi, gv = se.get_vector_by_id(pos)
        assert gi.dtype == np.uint32 and gv.dtype == np.float32
        assert gi.tobytes() == idx[off[pos]:off[pos + 1]].tobytes() and gv.tobytes() == val[off[pos]:off[pos + 1]].tobytes()
        seen.add(int(counts[pos]))
    assert {0, 1, 4096} <= seen
    assert se.get_vector_by_id(n) is None
    # the size query
    from zvec_amd import _lib
    c = C.c_uint32(77)
    assert _lib.lib().zvec_hip_sparse_get_vector(se._h, 0, C.byref(c), None, None) == 0 and c.value == 4096
    assert _lib.lib().zvec_hip_sparse_get_vector(se._h, n, C.byref(c), None, None) == NO_EXIST


@pytest.mark.parametrize("k", [10, 200])
def test_search_dev_equals_search(k):
    import torch
    n, nq = 1000, 130
    rows, queries, ref, A, m = R.make_case(n, nq, 100000, True)
    se = _index(rows)
    keys, scores, counts = _search(se, queries, k)
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(queries[1].view(np.int32).copy()).to(dev)
    d_val = torch.from_numpy(queries[2].copy()).to(dev)
    d_keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
    d_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d_counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    ctx = se.create_context()
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(2):            # (twice: the second call meets the first one's plan upload)
        assert se.search_dev(queries[0], d_idx.data_ptr(), d_val.data_ptr(), nq, k, d_keys.data_ptr(), d_scores.data_ptr(),
                             d_counts.data_ptr(), ctx, stream=ts.cuda_stream) == 0
    ts.synchronize()
    got_counts = d_counts.cpu().numpy().view(np.uint32)
    got_scores = d_scores.cpu().numpy()
    got_keys = d_keys.cpu().numpy().view(np.uint64)
    assert got_counts.tolist() == counts.tolist()
    for q in range(nq):
        c = int(counts[q])
        assert got_scores[q, :c].tobytes() == scores[q, :c].tobytes()
    R.check_sparse_lists(got_keys, got_scores, got_counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


def test_two_contexts_from_two_threads():
    n, nq, k = 5000, 130, 10
    rows, queries, ref, A, m = R.make_case(n, nq, 100000, True)
    se = _index(rows)
    single = _search(se, queries, k)
    out, errs = {}, []

    def work(i):
        try:
            ctx = se.create_context()
            for _ in range(3):
                out[i] = _search(se, queries, k, ctx=ctx)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs
    for i in range(2):
        keys, scores, counts = out[i]
        assert counts.tolist() == single[2].tolist()
        assert scores.tobytes() == single[1].tobytes()
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


def test_refusals():
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer()
    ok = (np.array([2, 0, 1], np.uint32), np.array([3, 9, 4], np.uint32), np.ones(3, np.float32))
    assert se.add_batch(*ok) == 0 and se.count() == 3
    # a row longer than 4096: InvalidArgument, and nothing of the call is stored
    long_idx = np.arange(4097, dtype=np.uint32)
    assert se.add_batch(np.array([1, 4097], np.uint32), np.concatenate([[5], long_idx]).astype(np.uint32),
                        np.ones(4098, np.float32)) == INVALID
    assert se.count() == 3 and se.element_count() == 3
    # indices must be strictly ascending inside a run (the reference's merge join requires it and checks nothing)
    assert se.add_batch(np.array([1, 2], np.uint32), np.array([7, 9, 8], np.uint32), np.ones(3, np.float32)) == INVALID
    assert se.add_batch(np.array([2], np.uint32), np.array([8, 8], np.uint32), np.ones(2, np.float32)) == INVALID
    assert se.count() == 3
    # ... while a new run may start below the end of the previous one
    assert se.add_batch(np.array([1, 1], np.uint32), np.array([9, 2], np.uint32), np.ones(2, np.float32)) == 0 and se.count() == 5
    ctx = se.create_context()
    ctx.set_topk(2)
    assert se.search_impl(np.array([4097], np.uint32), long_idx, np.ones(4097, np.float32), 1, ctx) == INVALID
    assert se.search_impl(np.array([2], np.uint32), np.array([5, 4], np.uint32), np.ones(2, np.float32), 1, ctx) == INVALID
    assert se.search_impl(np.array([2], np.uint32), np.array([5], np.uint32), np.ones(1, np.float32), 1, ctx) == INVALID
    assert se.search_impl(np.array([1], np.uint32), np.array([9], np.uint32), np.ones(1, np.float32), 1, ctx) == 0
    assert sorted(ctx.keys[0].tolist()) == [0, 3] and ctx.scores[0].tolist() == [-1.0, -1.0]
    # topk beyond the ABI bound
    ctx.set_topk(5119)
    assert se.search_impl(np.array([1], np.uint32), np.array([9], np.uint32), np.ones(1, np.float32), 1, ctx) == UNSUPPORTED
    ctx.set_topk(0)
    assert se.search_impl(np.array([1], np.uint32), np.array([9], np.uint32), np.ones(1, np.float32), 1, ctx) == INVALID
    # group-by stays with the reference
    ctx.set_topk(2)
    ctx.set_group_params(2, 2)
    ctx.set_group_by(lambda key: key % 2)
    assert se.search_impl(np.array([1], np.uint32), np.array([9], np.uint32), np.ones(1, np.float32), 1, ctx) == UNSUPPORTED


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sparse_search")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "sparse_search.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert out.stdout.decode().count("query") == 3
