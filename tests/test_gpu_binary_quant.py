"""fp32 rows and queries turned into sign bits on the GPU (BinaryConverter / BinaryReformer) and the Hamming index fed with them,
against tests/binary_quant_ref.py.  The outputs are integers or exact popcounts, so every comparison is bit for bit; only the
membership and order of EQUAL scores is left free (check_hamming_lists)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binary_quant_ref import binary_encode_reference, converter_encode_dims  # noqa: E402
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISMATCH, INVALID = -24, -31
GUARD = 0xA5C35A3C
DENORMAL = np.float32(1e-40)
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, DENORMAL, -DENORMAL, 0.25, -1.0], np.float32)


def _rows(rng, count, dim):
    """random normal rows with the special values at row starts, row ends and on both sides of every 32- and 64-value boundary"""
    rows = rng.standard_normal((count, dim)).astype(np.float32)
    spots = sorted({i for b in range(0, dim + 1, 32) for i in (b - 1, b) if 0 <= i < dim} | {0, dim - 1})
    for r in range(count):
        for j, i in enumerate(spots):
            rows[r, i] = SPECIALS[(r + j) % SPECIALS.size]
    return rows


def _words(dim):
    return (dim + 31) // 32


def _bits_index(dim, streamer=False, dtype="binary32"):
    import zvec_amd as zv
    return (zv.HipFlatStreamer if streamer else zv.HipFlatSearcher)(_words(dim) * 32, "Hamming", dtype=dtype)


# pairwise cover of count x dim; every case runs the three encode_dims and the three thresholds
ENCODER_CASES = [(1, 1), (3, 31), (64, 32), (65, 33), (257, 63), (1, 64), (3, 65), (64, 127), (65, 128), (257, 129), (1, 768), (3, 1000),
                 (64, 1), (65, 31), (257, 32), (1, 33), (3, 63), (64, 64), (65, 65), (257, 127), (1, 128), (3, 129), (64, 768), (65, 1000),
                 (257, 768), (257, 1000), (64, 33), (65, 64), (3, 32), (1, 127)]


@pytest.mark.parametrize("count,dim", ENCODER_CASES)
def test_encoder_against_the_restatement(count, dim):
    """host-pointer and device-pointer entries; the device output lies between guard words that must come back untouched"""
    import torch
    import zvec_amd as zv
    rng = np.random.default_rng(count * 1009 + dim)
    rows = _rows(rng, count, dim)
    ctx = zv.IndexContext(0)
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(rows).to(dev)
    words = _words(dim)
    for ed in sorted({dim, 1, converter_encode_dims(dim)}):
        if ed < 1 or ed > dim:
            continue
        for thr in (0.0, 0.25, -1.0):
            want = binary_encode_reference(rows, thr, ed)
            got = ctx.binary_encode(rows, thr, ed)
            assert np.array_equal(got, want), "host entry count=%d dim=%d encode_dims=%d threshold=%r" % (count, dim, ed, thr)
            buf = torch.full((count * words + 16,), GUARD - (1 << 32), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.binary_encode_dev(d_in.data_ptr(), count, dim, buf.data_ptr() + 8 * 4, thr, ed)
            ctx.synchronize()
            out = buf.cpu().numpy().view(np.uint32)
            assert np.all(out[:8] == GUARD) and np.all(out[-8:] == GUARD), "guard words count=%d dim=%d" % (count, dim)
            assert np.array_equal(out[8:-8].reshape(count, words), want), "device entry count=%d dim=%d encode_dims=%d threshold=%r" % (
                count, dim, ed, thr)


@pytest.mark.parametrize("dim", [1, 31, 33, 65, 127, 1001])
def test_rows_that_are_only_four_byte_aligned(dim):
    """dim % 4 != 0 and a buffer that starts 4 bytes past a 16-byte boundary: no row but row 0 of a multiple-of-4 shift is 16-byte aligned"""
    import torch
    import zvec_amd as zv
    assert dim % 4 != 0
    rng = np.random.default_rng(dim)
    count = 9
    rows = _rows(rng, count, dim)
    dev = torch.device("cuda:0")
    raw = torch.zeros(count * dim + 8, dtype=torch.float32, device=dev)
    raw[1:1 + count * dim] = torch.from_numpy(rows.reshape(-1)).to(dev)
    assert (raw.data_ptr() + 4) % 16 == 4
    words = _words(dim)
    out = torch.zeros(count * words, dtype=torch.int32, device=dev)
    ctx = zv.IndexContext(0)
    torch.cuda.synchronize()
    ctx.binary_encode_dev(raw.data_ptr() + 4, count, dim, out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(count, words), binary_encode_reference(rows))


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_add_batch_fp32_then_get_vector(n):
    dim = 100
    rng = np.random.default_rng(n)
    rows = _rows(rng, n, dim)
    keys = (rng.permutation(n) + 5000).astype(np.uint64)
    for thr, ed in ((0.0, None), (0.25, converter_encode_dims(dim))):
        want = binary_encode_reference(rows, thr, ed)
        a, b = _bits_index(dim), _bits_index(dim)
        assert a.add_batch_fp32(rows, keys, threshold=thr, encode_dims=ed) == 0
        assert b.add_batch(want, keys) == 0
        assert a.count() == b.count() == n
        assert np.array_equal(a.get_vectors_by_ids(np.arange(n)), want)
        assert np.array_equal(a.get_vector_by_id(n - 1), want[n - 1])
        # keys and positions are those of add_batch of the same words: the same search answers with the same keys
        q = want[:min(n, 3)]
        for se in (a, b):
            ctx = se.create_context()
            ctx.set_topk(min(n, 4))
            assert se.search_impl(q, q.shape[0], ctx) == 0
            check_hamming_lists(ctx.keys, ctx.scores, ctx.counts, hamming_reference(want, q), min(n, 4), key_of_row=keys)


def test_interleaved_bit_and_fp32_appends_keep_storage_order():
    import torch
    dim = 70
    rng = np.random.default_rng(5)
    parts = [_rows(rng, m, dim) for m in (3, 130, 1, 127, 200)]
    se = _bits_index(dim, streamer=True)
    dev = torch.device("cuda:0")
    keep = []
    for i, p in enumerate(parts):
        if i % 2 == 0:
            assert se.add_batch_fp32(p) == 0
        elif i == 1:
            assert se.add_batch(binary_encode_reference(p)) == 0
        else:                                              # the device-pointer form, only enqueued
            d = torch.from_numpy(p).to(dev)
            keep.append(d)
            torch.cuda.synchronize()
            assert se.add_batch_fp32_dev(d.data_ptr(), p.shape[0], dim) == 0
    allrows = np.concatenate(parts)
    want = binary_encode_reference(allrows)
    assert se.count() == allrows.shape[0]
    assert np.array_equal(se.get_vectors_by_ids(np.arange(allrows.shape[0])), want)
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search_impl_fp32(allrows[::50], len(allrows[::50]), ctx) == 0
    check_hamming_lists(ctx.keys, ctx.scores, ctx.counts, hamming_reference(want, want[::50]), 3)


SEARCH_CASES = [(1, 1, 32, 1), (129, 33, 96, 10), (1000, 257, 768, 12), (1000, 3, 1000, "n+5")]


@pytest.mark.parametrize("n,nq,dim,k", SEARCH_CASES)
def test_search_impl_fp32_equals_search_impl_of_the_restated_words(n, nq, dim, k):
    import torch
    k = n + 5 if k == "n+5" else k
    rng = np.random.default_rng(n + nq + dim)
    rows, q = _rows(rng, n, dim), _rows(rng, nq, dim)
    thr = 0.25
    base, qw = binary_encode_reference(rows, thr), binary_encode_reference(q, thr)
    ref = hamming_reference(base, qw)
    se = _bits_index(dim)
    assert se.add_batch_fp32(rows, threshold=thr) == 0
    keep = rng.random(n) < 0.5
    keep[int(np.argmin(ref[0]))] = False
    ex = np.zeros((n + 63) // 64, np.uint64)
    idx = np.nonzero(~keep)[0]
    np.bitwise_or.at(ex, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    radius = float(np.sort(ref[0])[min(n - 1, 5)])
    for exclude, threshold in ((None, None), (ex, None), (None, radius)):
        res = []
        for fp32 in (True, False):
            ctx = se.create_context()
            ctx.set_topk(k)
            if exclude is not None:
                ctx.set_exclude_bitset(exclude)
            if threshold is not None:
                ctx.set_threshold(threshold)
            assert (se.search_impl_fp32(q, nq, ctx, bin_threshold=thr) if fp32 else se.search_impl(qw, nq, ctx)) == 0
            check_hamming_lists(ctx.keys, ctx.scores, ctx.counts, ref, k, threshold=threshold, admissible=None if exclude is None else keep)
            res.append((ctx.scores.copy(), ctx.counts.copy()))
        # both routes: the same counts and — equal scores freed — the same score lists
        assert np.array_equal(res[0][1], res[1][1])
        for i in range(nq):
            assert np.array_equal(res[0][0][i, :res[0][1][i]], res[1][0][i, :res[1][1][i]])
    # the device-pointer entry equals the host entry
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    dk = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    ds = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    dc = torch.zeros((nq,), dtype=torch.int32, device=dev)
    ctx = se.create_context()
    torch.cuda.synchronize()
    assert se.search_fp32_dev(dq.data_ptr(), dim, nq, k, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx, bin_threshold=thr) == 0
    ctx.synchronize()
    gk, gs, gc = dk.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dc.cpu().numpy().view(np.uint32)
    check_hamming_lists(gk, gs, gc, ref, k)
    hctx = se.create_context()
    hctx.set_topk(k)
    assert se.search_impl_fp32(q, nq, hctx, bin_threshold=thr) == 0
    assert np.array_equal(gc, hctx.counts)
    for i in range(nq):
        assert np.array_equal(gs[i, :gc[i]], hctx.scores[i, :gc[i]])


def _exact_scores(metric, rows, q):
    r, x = rows.astype(np.float64), q.astype(np.float64)
    if metric == "InnerProduct":
        return -(x @ r.T)
    return ((x[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)


def _check_lists(keys, scores, counts, exact, key_of_row, k, admissible=None):
    """keys / scores / counts against exact [nq][n] scores (integers, exact in fp32): ascending, every key's score its own, nothing
    strictly better left out; equal scores free"""
    nq, n = exact.shape
    row_of = {int(key): i for i, key in enumerate(key_of_row)}
    for i in range(nq):
        ok = np.ones(n, bool) if admissible is None else admissible[i]
        want = np.sort(exact[i][ok])[:k]
        c = int(counts[i])
        assert c == want.size
        assert np.array_equal(scores[i, :c].astype(np.float64), want)
        got = [row_of[int(x)] for x in keys[i, :c]]
        assert len(set(got)) == c and all(ok[r] for r in got)
        assert np.array_equal(exact[i][got], want)


@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
def test_preselect_flat(metric):
    import zvec_amd as zv
    n, nq, dim, k = 700, 9, 70, 6
    rng = np.random.default_rng(31)
    rows = rng.integers(-7, 8, (n, dim)).astype(np.float32)            # small integers: every fp32 score is exact
    q = rng.integers(-7, 8, (nq, dim)).astype(np.float32)
    keys = (rng.permutation(n) + 10_000).astype(np.uint64)
    exact = _exact_scores(metric, rows, q)
    pre = zv.HipBinaryPreselectFlat(dim, metric)
    assert pre.add_batch(rows[:300], keys[:300]) == 0 and pre.add_batch(rows[300:], keys[300:]) == 0
    assert pre.count() == n and pre.bits.count() == n
    assert np.array_equal(pre.bits.get_vectors_by_ids(np.arange(n)), binary_encode_reference(rows))
    ham = hamming_reference(binary_encode_reference(rows), binary_encode_reference(q))
    # 1. the result is the fp32 index's listed-rows search over the binary stage's candidates
    refine = 5
    gk, gs, gc = (x.copy() for x in pre.search(q, k, refine))
    pos, cnt = pre.candidates
    assert pos.shape == (nq, k * refine)
    check_hamming_lists(pos.astype(np.uint64), np.take_along_axis(ham, pos.astype(np.int64), 1).astype(np.float32), cnt, ham, k * refine)
    cand = np.zeros((nq, n), bool)
    for i in range(nq):
        cand[i, pos[i, :cnt[i]]] = True
    _check_lists(gk, gs, gc, exact, keys, k, admissible=cand)
    ctx = pre.rows.create_context()
    ctx.set_topk(k)
    assert pre.rows.search_bf_by_p_keys_impl(q, [keys[pos[i, :cnt[i]]] for i in range(nq)], nq, ctx) == 0
    assert np.array_equal(ctx.counts, gc) and np.array_equal(ctx.scores, gs)
    _check_lists(ctx.keys, ctx.scores, ctx.counts, exact, keys, k, admissible=cand)
    # 2. k * refine >= n: the fp32 index's own full search
    gk, gs, gc = (x.copy() for x in pre.search(q, k, n // k + 1))
    assert pre.candidates[0].shape == (nq, n) and np.all(pre.candidates[1] == n)
    full = pre.rows.create_context()
    full.set_topk(k)
    assert pre.rows.search_impl(q, nq, full) == 0
    assert np.array_equal(full.counts, gc) and np.array_equal(full.scores, gs)
    _check_lists(gk, gs, gc, exact, keys, k)
    # 3. refine = 1: the binary stage's candidate set, re-ordered by the fp32 scores
    gk, gs, gc = (x.copy() for x in pre.search(q, k, 1))
    pos, cnt = pre.candidates
    for i in range(nq):
        assert cnt[i] == k == gc[i]
        assert set(gk[i].tolist()) == set(keys[pos[i]].tolist())
        assert np.array_equal(gs[i].astype(np.float64), np.sort(exact[i][pos[i]]))


def test_refusals():
    import torch
    import zvec_amd as zv
    from zvec_amd import _lib
    L = _lib.lib()
    dim, n, k = 70, 20, 3
    rng = np.random.default_rng(41)
    rows = _rows(rng, n, dim)
    ctx = zv.IndexContext(0)
    out = np.full((n, _words(dim)), GUARD, np.uint32)
    okeys, oscores, ocounts = np.full((n, k), 77, np.uint64), np.full((n, k), 77, np.float32), np.full(n, 77, np.uint32)

    def untouched():
        return np.all(out == GUARD) and np.all(okeys == 77) and np.all(oscores == 77) and np.all(ocounts == 77)

    f0 = C.c_float(0.0)
    big = C.c_float(3.4e38)
    # the encoder
    for d, ed in ((dim, 0), (dim, dim + 1), (0, 0), (0, 1), ((1 << 20) + 1, 1)):
        assert L.zvec_hip_binary_encode(ctx._h, rows.ctypes.data, n, d, ed, f0, out.ctypes.data) == INVALID
        assert L.zvec_hip_binary_encode_dev(ctx._h, rows.ctypes.data, n, d, ed, f0, out.ctypes.data, None) == INVALID
    assert L.zvec_hip_binary_encode(None, rows.ctypes.data, n, dim, dim, f0, out.ctypes.data) == INVALID
    assert L.zvec_hip_binary_encode(ctx._h, None, n, dim, dim, f0, out.ctypes.data) == INVALID
    assert L.zvec_hip_binary_encode(ctx._h, rows.ctypes.data, n, dim, dim, f0, None) == INVALID
    assert L.zvec_hip_binary_encode_dev(ctx._h, None, n, dim, dim, f0, out.ctypes.data, None) == INVALID
    assert L.zvec_hip_binary_encode_dev(ctx._h, rows.ctypes.data, n, dim, dim, f0, None, None) == INVALID
    assert L.zvec_hip_binary_encode(ctx._h, rows.ctypes.data, 0, dim, dim, f0, out.ctypes.data) == 0
    assert L.zvec_hip_binary_encode_dev(ctx._h, None, 0, dim, dim, f0, None, None) == 0
    assert untouched()
    # handles that do not pair with fp32 rows of `dim` values
    b64 = zv.HipFlatSearcher(128, "Hamming", dtype="binary64")
    fp = zv.HipFlatSearcher(dim, "SquaredEuclidean")
    narrow = zv.HipFlatSearcher(64, "Hamming", dtype="binary32")          # 70 values need 96 bits
    wide = zv.HipFlatSearcher(128, "Hamming", dtype="binary32")
    good = _bits_index(dim)
    assert good.add_batch_fp32(rows) == 0
    drows = torch.from_numpy(rows).to("cuda:0")
    torch.cuda.synchronize()
    for se in (b64, fp, narrow, wide):
        n0 = se.count()
        assert L.zvec_hip_flat_append_fp32(se._h, rows.ctypes.data, n, dim, dim, f0, None) == MISMATCH
        assert L.zvec_hip_flat_append_fp32_dev(se._h, drows.data_ptr(), n, dim, dim, f0, None, None) == MISMATCH
        assert L.zvec_hip_flat_append_fp32(se._h, rows.ctypes.data, 0, dim, dim, f0, None) == MISMATCH
        assert L.zvec_hip_flat_search_fp32(se._h, None, rows.ctypes.data, dim, f0, n, k, big, None, okeys.ctypes.data, oscores.ctypes.data,
                                           ocounts.ctypes.data) == MISMATCH
        assert L.zvec_hip_flat_search_fp32_dev(se._h, None, drows.data_ptr(), dim, f0, n, k, big, None, okeys.ctypes.data,
                                               oscores.ctypes.data, ocounts.ctypes.data, None) == MISMATCH
        assert se.count() == n0
    # arguments out of range on a handle that pairs
    for d, ed in ((dim, 0), (dim, dim + 1), (0, 0), (0, 1)):
        assert L.zvec_hip_flat_append_fp32(good._h, rows.ctypes.data, n, d, ed, f0, None) == INVALID
        assert L.zvec_hip_flat_append_fp32_dev(good._h, drows.data_ptr(), n, d, ed, f0, None, None) == INVALID
    assert L.zvec_hip_flat_append_fp32(good._h, None, n, dim, dim, f0, None) == INVALID
    assert L.zvec_hip_flat_append_fp32_dev(good._h, None, n, dim, dim, f0, None, None) == INVALID
    assert L.zvec_hip_flat_append_fp32(None, rows.ctypes.data, n, dim, dim, f0, None) == INVALID
    assert L.zvec_hip_flat_append_fp32(good._h, None, 0, dim, dim, f0, None) == 0
    assert L.zvec_hip_flat_append_fp32_dev(good._h, None, 0, dim, dim, f0, None, None) == 0
    assert good.count() == n
    args = (okeys.ctypes.data, oscores.ctypes.data, ocounts.ctypes.data)
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, 0, f0, n, k, big, None, *args) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, None, dim, f0, n, k, big, None, *args) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, dim, f0, n, k, big, None, None, args[1], args[2]) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, dim, f0, n, k, big, None, args[0], None, args[2]) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, dim, f0, n, k, big, None, args[0], args[1], None) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, dim, f0, n, 0, big, None, *args) == INVALID
    assert L.zvec_hip_flat_search_fp32(None, None, rows.ctypes.data, dim, f0, n, k, big, None, *args) == INVALID
    assert L.zvec_hip_flat_search_fp32_dev(good._h, None, None, dim, f0, n, k, big, None, *args, None) == INVALID
    assert L.zvec_hip_flat_search_fp32_dev(good._h, None, drows.data_ptr(), 0, f0, n, k, big, None, *args, None) == INVALID
    assert L.zvec_hip_flat_search_fp32(good._h, None, rows.ctypes.data, dim, f0, 0, k, big, None, *args) == 0
    assert L.zvec_hip_flat_search_fp32_dev(good._h, None, drows.data_ptr(), dim, f0, 0, k, big, None, *args, None) == 0
    assert untouched()
    # the Python layer hands the codes through
    assert b64.add_batch_fp32(rows) == MISMATCH and fp.add_batch_fp32(rows) == MISMATCH
    assert good.add_batch_fp32(rows, encode_dims=dim + 1) == INVALID
    c2 = good.create_context()
    c2.set_topk(k)
    assert narrow.search_impl_fp32(rows, n, c2) == MISMATCH
    assert good.count() == n


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "binary_quantize")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "binary_quantize.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert out.stdout.decode().count("query") == 3
