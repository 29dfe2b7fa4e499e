"""Binary rows under the Hamming metric on the GPU (flat index), against tests/hamming_ref.py.  Scores are exact integers, so
every comparison is bit-exact; only the membership and order of EQUAL scores is left free (check_hamming_lists)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, MISMATCH, INVALID = -12, -24, -31


def _bits(rng, n, dim, dtype="binary32"):
    words = rng.integers(0, 2**32, (n, dim // 32), dtype=np.uint64).astype(np.uint32)
    return words if dtype == "binary32" else np.ascontiguousarray(words).view(np.uint64)


def _index(base, dim, dtype="binary32", streamer=False):
    import zvec_amd as zv
    se = (zv.HipFlatStreamer if streamer else zv.HipFlatSearcher)(dim, "Hamming", dtype=dtype)
    if len(base):
        assert se.add_batch(base) == 0
    return se


def _search(se, q, k, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    assert se.search_impl(q, q.shape[0], ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


# pairwise cover of n x queries x dim x k at the edges of the 128-row tile, the 32-query block and the word loop (4 + 2 + 1 chunks)
CASES = [
    (1, 1, 32, 1), (1, 31, 96, 10), (1, 33, 128, "n+5"), (1, 257, 768, 11),
    (127, 1, 96, 11), (127, 31, 32, "n+5"), (127, 33, 1056, 1), (127, 257, 128, 12),
    (128, 1, 128, 12), (128, 31, 768, 100), (128, 33, 32, 10), (128, 257, 96, "n+5"),
    (129, 1, 768, "n+5"), (129, 31, 1056, 12), (129, 33, 96, 100), (129, 257, 32, 11),
    (1000, 1, 1056, 100), (1000, 31, 128, 1), (1000, 33, 768, 12), (1000, 257, 96, 10),
    (5000, 1, 32, 10), (5000, 31, 96, 12), (5000, 33, 128, 11), (5000, 257, 1056, 10),
    (5000, 33, 768, "n+5"), (1000, 257, 32, 100), (5000, 31, 768, 1), (129, 1, 128, 10),
    (1000, 31, 1056, 11), (128, 33, 96, 1),
]


@pytest.mark.parametrize("n,nq,dim,k", CASES)
def test_random_bits_binary32(n, nq, dim, k):
    k = n + 5 if k == "n+5" else k
    rng = np.random.default_rng(n * 7 + nq * 3 + dim)
    base, q = _bits(rng, n, dim), _bits(rng, nq, dim)
    if k > 1000:
        q = q[:3]                      # (the dense route: a few queries show all of it)
    se = _index(base, dim)
    keys, scores, counts = _search(se, q, k)
    check_hamming_lists(keys, scores, counts, hamming_reference(base, q), k, what="n=%d nq=%d dim=%d k=%d" % (n, q.shape[0], dim, k))


@pytest.mark.parametrize("n,nq,dim,k", [(129, 33, 64, 10), (1000, 5, 192, 12), (127, 1, 192, 200)])
def test_random_bits_binary64(n, nq, dim, k):
    rng = np.random.default_rng(n + dim)
    base, q = _bits(rng, n, dim, "binary64"), _bits(rng, nq, dim, "binary64")
    assert base.dtype == np.uint64 and base.shape[1] == dim // 64
    se = _index(base, dim, "binary64")
    keys, scores, counts = _search(se, q, k)
    check_hamming_lists(keys, scores, counts, hamming_reference(base, q), k)
    assert np.array_equal(se.get_vectors_by_ids(np.arange(min(n, 70))), base[:70])


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(70)
    base, q = _bits(rng, 70_000, 96), _bits(rng, 8, 96)
    return _index(base, 96), base, q, hamming_reference(base, q)


def test_seventy_thousand_rows(big):
    se, base, q, ref = big
    keys, scores, counts = _search(se, q, 10)
    check_hamming_lists(keys, scores, counts, ref, 10)


def test_seventy_thousand_rows_keep_five_percent(big):
    se, base, q, ref = big
    keep = np.random.default_rng(5).random(70_000) < 0.05
    keys, scores, counts = _search(se, q, 10, exclude=_words_of(~keep))
    check_hamming_lists(keys, scores, counts, ref, 10, admissible=keep)


@pytest.mark.parametrize("k", [10, 768])
def test_planted_distances_without_ties(k):
    n = dim = 768
    rng = np.random.default_rng(11)
    q = _bits(rng, 1, dim)
    qbits = np.unpackbits(q.view(np.uint8), bitorder="little")
    rows = np.empty((n, dim // 32), np.uint32)
    for i in range(n):                                 # row i: the query with exactly i + 1 bits flipped
        b = qbits.copy()
        b[rng.choice(dim, i + 1, replace=False)] ^= 1
        rows[i] = np.packbits(b, bitorder="little").view(np.uint32)
    perm = rng.permutation(n)
    base = rows[perm]
    ref = hamming_reference(base, q)
    assert sorted(ref[0]) == list(range(1, n + 1))
    se = _index(base, dim)
    keys, scores, counts = _search(se, q, k)
    assert counts[0] == k
    assert np.array_equal(keys[0], np.argsort(ref[0])[:k].astype(np.uint64))
    assert np.array_equal(scores[0], np.arange(1, k + 1, dtype=np.float32))


def test_all_equal_scores():
    rng = np.random.default_rng(12)
    row = _bits(rng, 1, 128)
    base = np.repeat(row, 300, axis=0)
    q = _bits(rng, 2, 128)
    se = _index(base, 128)
    keys, scores, counts = _search(se, q, 10)
    ref = hamming_reference(base, q)
    check_hamming_lists(keys, scores, counts, ref, 10)
    for i in range(2):
        assert counts[i] == 10 and len(set(keys[i].tolist())) == 10 and keys[i].max() < 300
        assert np.all(scores[i] == np.float32(ref[i, 0]))


def test_large_k_dense_route():
    rng = np.random.default_rng(13)
    base, q = _bits(rng, 5000, 128), _bits(rng, 3, 128)
    se = _index(base, 128)
    keys, scores, counts = _search(se, q, 2000)
    check_hamming_lists(keys, scores, counts, hamming_reference(base, q), 2000)


def test_threshold():
    rng = np.random.default_rng(14)
    base, q = _bits(rng, 1000, 96), _bits(rng, 5, 96)
    ref = hamming_reference(base, q)
    se = _index(base, 96)
    r = int(np.sort(ref[0])[20])                        # an occurring score
    for radius in (r, r - 1, float(r) - 0.5):
        keys, scores, counts = _search(se, q, 100, threshold=float(radius))
        check_hamming_lists(keys, scores, counts, ref, 100, threshold=float(radius))
    keys, scores, counts = _search(se, q, 100, threshold=float(r))
    assert scores[0, counts[0] - 1] == r                # the radius itself is kept ...
    keys, scores, counts = _search(se, q, 100, threshold=float(r - 1))
    assert counts[0] == 0 or scores[0, counts[0] - 1] < r      # ... one below drops it
    keys, scores, counts = _search(se, q, 10, threshold=float(ref.min() - 1))
    assert np.all(counts == 0)


def test_exclude_bitset():
    rng = np.random.default_rng(15)
    base, q = _bits(rng, 1000, 128), _bits(rng, 33, 128)
    ref = hamming_reference(base, q)
    se = _index(base, 128)
    keep = rng.random(1000) < 0.1
    all_but_best = np.ones(1000, bool)
    all_but_best[int(np.argmin(ref[0]))] = False
    for adm in (keep, all_but_best):
        keys, scores, counts = _search(se, q, 12, exclude=_words_of(~adm))
        check_hamming_lists(keys, scores, counts, ref, 12, admissible=adm)
    keys, scores, counts = _search(se, q, 12, exclude=_words_of(np.ones(1000, bool)))
    assert np.all(counts == 0)


def test_holes_overwrites_and_round_trip():
    rng = np.random.default_rng(16)
    dim = 96
    ids = np.array([0, 1, 2, 5, 6, 200, 201, 330], np.uint32)
    rows = _bits(rng, ids.size, dim)
    se = _index(np.zeros((0, dim // 32), np.uint32), dim, streamer=True)
    assert se.add_with_id_batch(ids, rows) == 0
    assert se.count() == 331 and se.holes() == 331 - ids.size
    new = _bits(rng, 3, dim)
    assert se.add_with_id_batch(np.array([1, 200, 3], np.uint32), new) == 0       # two overwrites, one hole filled
    assert se.add_with_id_impl(5, new[0]) == 0                                      # a third overwrite, a document at a time
    assert se.holes() == 331 - ids.size - 1
    stored = np.zeros((331, dim // 32), np.uint32)
    stored[ids] = rows
    stored[[1, 200, 3]] = new
    stored[5] = new[0]
    live = np.zeros(331, bool)
    live[ids] = True
    live[3] = True
    assert np.array_equal(se.get_vectors_by_ids(np.nonzero(live)[0]), stored[live])
    assert np.array_equal(se.get_vector_by_id(200), new[1])
    q = np.concatenate([new, _bits(rng, 2, dim), np.zeros((1, dim // 32), np.uint32)])      # (the zero query is closest to the holes' zero rows)
    ref = hamming_reference(stored, q)
    for k in (4, 400):
        keys, scores, counts = _search(se, q, k)
        check_hamming_lists(keys, scores, counts, ref, k, admissible=live)


def test_search_by_ids():
    rng = np.random.default_rng(17)
    dim = 128
    ids = np.concatenate([np.arange(300), [305]]).astype(np.uint32)       # positions 300..304 are holes
    rows = _bits(rng, ids.size, dim)
    se = _index(np.zeros((0, dim // 32), np.uint32), dim, streamer=True)
    assert se.add_with_id_batch(ids, rows) == 0
    stored = np.zeros((306, dim // 32), np.uint32)
    stored[ids] = rows
    q = _bits(rng, 4, dim)
    ref = hamming_reference(stored, q)
    lists = [list(range(10, 60)), [], [299, 302, 305, 7], list(range(0, 300, 3))]        # longer than k, empty, naming a hole, long
    offs = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
    flat = np.asarray([p for l in lists for p in l] or [0], np.uint32)
    k = 12
    keys, scores, counts = np.zeros((4, k), np.uint64), np.zeros((4, k), np.float32), np.zeros(4, np.uint32)
    from zvec_amd import _lib
    rc = _lib.lib().zvec_hip_flat_search_by_ids(se._h, None, q.ctypes.data, 4, flat.ctypes.data, offs.ctypes.data, k, C.c_float(3.4e38), None,
                                                keys.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    assert rc == 0
    adm = np.zeros((4, 306), bool)
    for i, l in enumerate(lists):
        adm[i, [p for p in l if p < 300 or p == 305]] = True
    check_hamming_lists(keys, scores, counts, ref, k, admissible=adm)
    assert counts[1] == 0 and counts[2] == 3


def test_batch_distance():
    rng = np.random.default_rng(18)
    base, q = _bits(rng, 2000, 192), _bits(rng, 1, 192)
    se = _index(base, 192)
    pos = rng.choice(2000, 500, replace=False).astype(np.uint32)
    pos[123] = 2000                                     # beyond the count: +inf, as on the fp path
    got = se.batch_distance(q, pos)
    want = hamming_reference(base, q)[0][np.minimum(pos, 1999)].astype(np.float32)
    want[123] = np.inf
    assert np.array_equal(got, want)


def test_search_dev_on_a_callers_stream():
    import torch
    rng = np.random.default_rng(19)
    base, q = _bits(rng, 3000, 96), _bits(rng, 40, 96)
    ref = hamming_reference(base, q)
    se = _index(base, 96)
    k = 10
    hk, hs, hc = _search(se, q, k)
    check_hamming_lists(hk, hs, hc, ref, k)
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q.view(np.int32)).to(dev)
    dk = torch.zeros((40, k), dtype=torch.int64, device=dev)
    ds = torch.zeros((40, k), dtype=torch.float32, device=dev)
    dc = torch.zeros((40,), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx = se.create_context()
    assert se.search_dev(dq.data_ptr(), 40, k, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx, stream=stream.cuda_stream) == 0
    stream.synchronize()
    check_hamming_lists(dk.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dc.cpu().numpy().view(np.uint32), ref, k)
    assert np.array_equal(ds.cpu().numpy(), hs)
    # rows appended from a device pointer are searched like the others
    extra = _bits(rng, 130, 96)
    de = torch.from_numpy(extra.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    assert se.add_batch_dev(de.data_ptr(), 130) == 0
    hk, hs, hc = _search(se, q, k)
    check_hamming_lists(hk, hs, hc, hamming_reference(np.concatenate([base, extra]), q), k)


def test_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.zvec_hip_flat_create(96, _lib.DT_BINARY32, _lib.METRIC_L2, 0, C.byref(h)) == MISMATCH
    assert L.zvec_hip_flat_create(96, _lib.DT_FP32, _lib.METRIC_HAMMING, 0, C.byref(h)) == MISMATCH
    assert L.zvec_hip_flat_create(96, _lib.DT_FP16, _lib.METRIC_HAMMING, 0, C.byref(h)) == MISMATCH
    assert L.zvec_hip_flat_create(48, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_flat_create(96, _lib.DT_BINARY64, _lib.METRIC_HAMMING, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_flat_create((1 << 20) + 32, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_ivf_create(96, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(h)) == UNSUPPORTED
    dev = (C.c_int * 1)(0)
    assert L.zvec_hip_shards_create(96, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, dev, 1, C.byref(h)) == UNSUPPORTED
    rng = np.random.default_rng(20)
    base = _bits(rng, 200, 96)
    se = _index(base, 96)
    assert L.zvec_hip_flat_set_shadow(se._h, 1, 0) == UNSUPPORTED
    assert L.zvec_hip_flat_shadow_info(se._h, None, None, None, None) == UNSUPPORTED
    w = C.c_uint32(0)
    assert L.zvec_hip_flat_shadow_width(se._h, 10, C.byref(w)) == UNSUPPORTED
    assert se.load_features(base.tobytes(), 200) == UNSUPPORTED
    blocks = np.zeros(4096, np.uint8)
    keep = np.ones(1, np.uint32)
    assert L.zvec_hip_flat_load_blocks(se._h, blocks.ctypes.data, 4096, 1, 4096, 8, keep.ctypes.data) == UNSUPPORTED
    ctx = se.create_context()
    ctx.set_group_params(2, 2)
    ctx.set_group_by(lambda key: key % 3)
    assert se.search_impl(base[:2], 2, ctx) == UNSUPPORTED
    assert se.search_bf_by_p_keys_impl(base[:2], [[1, 2], [3]], 2, ctx) == UNSUPPORTED
    # a filter built on the GPU serves a binary index like any other
    words = se.build_filter(zv.DocFilter(forward=np.arange(200) % 2 == 0))
    adm = np.arange(200) % 2 == 0
    keys, scores, counts = _search(se, base[:3], 5, exclude=words)
    check_hamming_lists(keys, scores, counts, hamming_reference(base, base[:3]), 5, admissible=adm)


def test_c_example_runs():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hamming_search")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "hamming_search.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert out.stdout.decode().count("query") == 3


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_fp_results_unchanged_around_a_hamming_search(dtype):
    """one context serves an fp index, then a binary one, then the fp one again: the shared workspace hands the fp search the same bytes"""
    import zvec_amd as zv
    rng = np.random.default_rng(21)
    npdt = np.float16 if dtype == "fp16" else np.float32
    base = rng.integers(-8, 8, (1000, 64)).astype(npdt)
    q = rng.integers(-8, 8, (20, 64)).astype(npdt)
    fp = zv.HipFlatSearcher(64, "SquaredEuclidean", dtype=dtype)
    assert fp.load(base) == 0
    bits, bq = _bits(rng, 1000, 96), _bits(rng, 20, 96)
    ham = _index(bits, 96)
    ctx = fp.create_context()
    ctx.set_topk(10)
    assert fp.search_impl(q, 20, ctx) == 0
    before = (ctx.keys.tobytes(), ctx.scores.tobytes(), ctx.counts.tobytes())
    assert ham.search_impl(bq, 20, ctx) == 0
    check_hamming_lists(ctx.keys, ctx.scores, ctx.counts, hamming_reference(bits, bq), 10)
    assert fp.search_impl(q, 20, ctx) == 0
    assert (ctx.keys.tobytes(), ctx.scores.tobytes(), ctx.counts.tobytes()) == before
