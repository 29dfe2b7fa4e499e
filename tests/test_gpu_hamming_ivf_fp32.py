"""The Hamming IVF index fed with fp32 on the GPU (zvec_hip_bivf_build_fp32 / _attach_rows / _search_fp32 / _last_candidates),
against tests/hamming_ivf_fp32_ref.py.  Every search is checked in two steps: stage 1 — the Hamming candidates read back — by the
rule of Hamming lists, and stage 2 given those candidates: bit for bit on integer-valued data, within the derived band of the fp64
score on real-valued data.  Output arrays are filled with sentinels first: nothing beyond a query's count may be written."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ivf_fp32_ref as F  # noqa: E402
import hamming_ivf_ref as R  # noqa: E402
from binary_quant_ref import binary_encode_reference  # noqa: E402
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, MISMATCH, INVALID, NO_INDEX_LOADED, NO_READY, NO_EXIST = -12, -24, -31, -204, -21, -22
NO_CUT = 0xffffffff
FLT_MAX = float(np.finfo(np.float32).max)
KEY_SENTINEL, SCORE_SENTINEL, COUNT_SENTINEL = 0xabababababababab, np.float32(-777.0), 0xcdcdcdcd


def _searcher(dim, dtype="binary32"):
    import zvec_amd as zv
    return zv.HipHammingIVFSearcher(F.dim_bits(dim), dtype=dtype)


def _attached(cent, offs, rows, frows, dim, metric, keys=None):
    se = _searcher(dim)
    assert se.load(cent, offs, rows, keys) == 0
    assert se.rows_info() == (0, 0, 0)
    assert se.attach_rows(frows, metric) == 0
    from zvec_amd.index import metric_from_name
    assert se.rows_info() == (dim, metric_from_name(metric), rows.shape[0] * dim * 4)
    return se


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(se, ctx, qf, topk, refine, nprobe, max_scan=NO_CUT, threshold=FLT_MAX, exclude=None, bin_threshold=0.0, dim=None):
    """zvec_hip_bivf_search_fp32 into sentinel-filled outputs: (rc, keys, scores, counts)"""
    from zvec_amd import _lib
    n = qf.shape[0]
    keys = np.full((n, topk), KEY_SENTINEL, np.uint64)
    scores = np.full((n, topk), SCORE_SENTINEL, np.float32)
    counts = np.full(n, COUNT_SENTINEL, np.uint32)
    ex = None if exclude is None else R.words_of(exclude)
    rc = _lib.lib().zvec_hip_bivf_search_fp32(
        se._h, ctx._h, _ptr(qf), n, qf.shape[1] if dim is None else dim, topk, refine, threshold, bin_threshold, nprobe, max_scan,
        None if ex is None else ex.ctypes.data_as(C.POINTER(C.c_uint64)), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
        scores.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
    return rc, keys, scores, counts


def _untouched(keys, scores, counts):
    return bool(np.all(keys == KEY_SENTINEL) and np.all(scores == SCORE_SENTINEL) and np.all(counts == COUNT_SENTINEL))


def _check_outputs(got, cand, fx, metric, topk, kc, nprobe, integer, max_scan=NO_CUT, threshold=None, exclude=None, keys=None, what=""):
    """both checkers on one search's outputs and its read-back candidates; returns the ambiguous queries (real data)"""
    cent, offs, rows, frows, qf, qbits = fx
    gk, gs, gc = got
    pos, ham, cnt = cand
    F.check_stage1(pos, ham, cnt, cent, offs, rows, qbits, kc, nprobe, max_scan, exclude, what=what)
    beyond = np.arange(topk)[None, :] >= gc[:, None]
    assert np.all(gk[beyond] == KEY_SENTINEL) and np.all(gs[beyond] == SCORE_SENTINEL), what + ": written beyond the count"
    if integer:
        F.check_stage2_exact(gk, gs, gc, pos, cnt, frows, qf, metric, topk, threshold, keys, what=what)
        return 0
    amb = F.check_stage2_real(gk, gs, gc, pos, cnt, frows, qf, metric, topk, threshold, keys, what=what)
    assert amb * 20 <= max(qf.shape[0], 20), "%s: %d ambiguous queries of %d" % (what, amb, qf.shape[0])
    return amb


def _check(se, fx, metric, topk, refine, nprobe, integer, max_scan=NO_CUT, threshold=None, exclude=None, keys=None, what="", ctx=None):
    ctx = ctx or se.create_context()
    kc = F.kc_of(topk, refine)
    rc, gk, gs, gc = _raw(se, ctx, fx[4], topk, refine, nprobe, max_scan, FLT_MAX if threshold is None else threshold, exclude)
    assert rc == 0, what
    cand = se.last_candidates(ctx, fx[4].shape[0], kc)
    _check_outputs((gk, gs, gc), cand, fx, metric, topk, kc, nprobe, integer, max_scan, threshold, exclude, keys, what)
    return gk, gs, gc, cand


# ---- build ------------------------------------------------------------------------------------------------------------------------
def _export_bytes(se):
    return tuple(a.tobytes() for a in se.export())


def test_build_fp32_equals_build_of_the_encoded_rows():
    import torch
    rng = np.random.default_rng(600)
    n, dim, nlist = 600, 100, 7
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    bits = binary_encode_reference(rows)
    plain, host, dev = _searcher(dim), _searcher(dim), _searcher(dim)
    assert plain.build(bits, nlist, kmeans_iters=3, seed=5) == 0
    assert host.build_fp32(rows, nlist, F.L2, kmeans_iters=3, seed=5) == 0
    d = torch.from_numpy(rows).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.build_fp32_dev(d.data_ptr(), n, dim, nlist, F.L2, kmeans_iters=3, seed=5) == 0
    assert _export_bytes(host) == _export_bytes(plain) and _export_bytes(dev) == _export_bytes(plain)
    cent, offs, row_ids = host.export()
    assert len(set(row_ids.tolist())) == n
    for se in (host, dev):
        assert se.info() == (n, nlist) and se.rows_info() == (dim, 0, n * dim * 4)
        got = se.get_rows_by_ids(np.arange(n))
        assert np.array_equal(got.view(np.uint32), rows[row_ids.astype(np.int64)].view(np.uint32))
        assert np.array_equal(se.get_vectors_by_ids(np.arange(n)), bits[row_ids.astype(np.int64)])
    assert plain.rows_info() == (0, 0, 0)
    # a search on the built index: keys are original row numbers
    qf = rows[:10] + np.float32(0.25) * rng.standard_normal((10, dim)).astype(np.float32)
    order = row_ids.astype(np.int64)
    fx = (cent, offs, bits[order], rows[order], qf, binary_encode_reference(qf))
    gk, _, gc, cand = _check(host, fx, F.L2, 5, 4, 3, False, keys=row_ids, what="built")
    assert np.all(gc == 5)
    for i in range(10):                                                     # the query's own row wins wherever it is a candidate
        if i in row_ids[cand[0][i, :cand[2][i]].astype(np.int64)]:
            assert gk[i, 0] == i
    # a threshold of the encoder other than 0
    t = _searcher(dim)
    assert t.build_fp32(rows, nlist, F.IP, kmeans_iters=1, seed=5, bin_threshold=0.5) == 0
    assert np.array_equal(t.get_vectors_by_ids(np.arange(n)), binary_encode_reference(rows, 0.5)[t.export()[2].astype(np.int64)])
    # the next plain build drops the rows
    assert host.build(bits, nlist, kmeans_iters=1, seed=5) == 0 and host.rows_info() == (0, 0, 0)


# ---- attach_rows + search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [96, 100, 33])
@pytest.mark.parametrize("integer", [True, False])
def test_attach_rows_and_search(dim, integer):
    """dim 96: 16-byte row loads; 100 and 33: dword loads (33: rows shorter than a wave); 40 queries: a second query block"""
    fx = F.fp_index(np.random.default_rng(dim), dim, R.RAGGED, integer)
    cent, offs, rows, frows, qf, qbits = fx
    keys = (np.arange(rows.shape[0], dtype=np.uint64) * 7 + 1000)
    for metric in (F.L2, F.IP):
        se = _attached(cent, offs, rows, frows, dim, metric, keys)
        assert np.array_equal(se.get_rows_by_ids([0, 127, 128, 684]).view(np.uint32), frows[[0, 127, 128, 684]].view(np.uint32))
        for nprobe in (1, 3, len(R.RAGGED)):
            _check(se, fx, metric, 5, 4, nprobe, integer, keys=keys, what="dim=%d %s nprobe=%d" % (dim, metric, nprobe))


def test_attach_again_replaces_the_rows_and_the_python_layer_fills_the_context():
    fx = F.fp_index(np.random.default_rng(7), 100, R.RAGGED, True)
    cent, offs, rows, frows, qf, qbits = fx
    se = _attached(cent, offs, rows, frows, 100, F.L2)
    other = np.ascontiguousarray(frows[::-1])
    assert se.attach_rows(other, F.IP) == 0 and se.rows_info()[1] == 1
    assert np.array_equal(se.get_rows_by_ids(np.arange(685)), other)
    ctx = se.create_context()
    ctx.set_topk(5)
    assert se.search_impl_fp32(qf, 40, ctx, refine=4, nprobe=3, max_scan=NO_CUT) == 0
    cand = se.last_candidates(ctx, 40, 20)
    F.check_stage1(*cand, cent, offs, rows, qbits, 20, 3)
    F.check_stage2_exact(ctx.keys, ctx.scores, ctx.counts, cand[0], cand[2], other, qf, F.IP, 5)
    assert [len(ctx.result(i)) for i in range(40)] == [int(c) for c in ctx.counts]


@pytest.mark.parametrize("topk,refine", [(40, 8), (128, 1), (1, 1)])
def test_clamp_and_widths(topk, refine):
    """topk * refine beyond 128 is clamped to kc = 128; topk = 128 leaves nothing to refine"""
    fx = F.fp_index(np.random.default_rng(topk), 96, R.RAGGED, True, nq=9)
    se = _attached(*fx[:4], 96, F.L2)
    kc = F.kc_of(topk, refine)
    assert kc == min(128, topk * refine)
    _, _, gc, cand = _check(se, fx, F.L2, topk, refine, len(R.RAGGED), True, what="topk=%d refine=%d" % (topk, refine))
    assert np.all(cand[2] == kc) and np.all(gc == topk)


def test_fewer_candidates_than_topk():
    *fx, lst = F.short_list(np.random.default_rng(5))
    se = _attached(*fx[:4], 100, F.L2)
    gk, gs, gc, cand = _check(se, tuple(fx), F.L2, 5, 4, 1, True)
    assert np.all(gc == 3) and np.all(cand[2] == 3)
    assert np.all(gk[:, 3:] == KEY_SENTINEL) and np.all(gs[:, 3:] == SCORE_SENTINEL)


def test_exclude_and_radius():
    rng = np.random.default_rng(11)
    fx = F.fp_index(rng, 100, R.RAGGED, True)
    cent, offs, rows, frows, qf, qbits = fx
    se = _attached(cent, offs, rows, frows, 100, F.L2)
    _, gs, _, cand = _check(se, fx, F.L2, 5, 4, 3, True)
    # exclude bits apply in stage 1: every first candidate of the plain search, and a random third of the rows
    exclude = rng.random(rows.shape[0]) < 0.33
    exclude[cand[0][:, 0]] = True
    _, _, _, cand_ex = _check(se, fx, F.L2, 5, 4, 3, True, exclude=exclude, what="exclude")
    assert not exclude[cand_ex[0][cand_ex[0] != F.IDX_NONE]].any()
    # the radius applies on the fp32 score: the median third score cuts some queries short, not all
    thr = float(np.median(gs[:, 2]))
    _, _, gc, cand_thr = _check(se, fx, F.L2, 5, 4, 3, True, threshold=thr, what="radius")
    assert gc.min() < 5 and gc.max() >= 3
    assert np.all(cand_thr[2] == cand[2])                                  # (stage 1 has no radius)
    # every candidate beyond the radius: the count is 0
    _, _, gc, _ = _check(se, fx, F.L2, 5, 4, 3, True, threshold=-1.0, what="radius below every score")
    assert not gc.any()
    # both at once under IP (scores are negative there: the radius is a plain fp32 compare)
    se_ip = _attached(cent, offs, rows, frows, 100, F.IP)
    _, gs_ip, _, _ = _check(se_ip, fx, F.IP, 5, 4, 3, True, exclude=exclude)
    _check(se_ip, fx, F.IP, 5, 4, 3, True, exclude=exclude, threshold=float(np.median(gs_ip[:, 1])), what="ip exclude radius")


def test_max_scan_count_cuts_the_probe_list():
    *fx, nprobe, length = F.max_scan_case(np.random.default_rng(4))
    fx = tuple(fx)
    se = _attached(*fx[:4], 96, F.L2)
    for max_scan in (length, length + 1, 1, NO_CUT):
        _check(se, fx, F.L2, 5, 4, nprobe, True, max_scan=max_scan, what="max_scan=%d" % max_scan)
    ctx = se.create_context()
    rc, gk, gs, gc = _raw(se, ctx, fx[4], 5, 4, nprobe, max_scan=0)
    assert rc == 0 and not gc.any() and np.all(gk == KEY_SENTINEL) and not se.last_candidates(ctx, 6, 20)[2].any()


def test_two_slices():
    from zvec_amd import _lib
    *fx, nprobe, topk, refine, cap = F.two_slices(np.random.default_rng(6))
    fx = tuple(fx)
    se = _attached(*fx[:4], 100, F.L2)
    one_k, one_s, one_c, one_cand = _check(se, fx, F.L2, topk, refine, nprobe, True)
    L = _lib.lib()
    before = C.c_int(0)
    assert L.zvec_hip_get_option(b"bivf_part_bytes", C.byref(before)) == 0
    assert L.zvec_hip_set_option(b"bivf_part_bytes", cap) == 0
    try:
        two_k, two_s, two_c, two_cand = _check(se, fx, F.L2, topk, refine, nprobe, True, what="two slices")
    finally:
        assert L.zvec_hip_set_option(b"bivf_part_bytes", before.value) == 0
    assert np.array_equal(one_c, two_c) and np.array_equal(one_cand[1], two_cand[1]) and np.array_equal(one_cand[2], two_cand[2])


def test_dev_entries():
    import torch
    fx = F.fp_index(np.random.default_rng(21), 100, R.RAGGED, True)
    cent, offs, rows, frows, qf, qbits = fx
    dev = torch.device("cuda:0")
    se = _searcher(100)
    assert se.load(cent, offs, rows) == 0
    drows = torch.from_numpy(frows).to(dev)
    torch.cuda.synchronize()
    assert se.attach_rows_dev(drows.data_ptr(), 100, F.IP) == 0
    assert np.array_equal(se.get_rows_by_ids(np.arange(685)), frows)
    topk, refine, nprobe, kc = 5, 4, 3, 20
    exclude = np.random.default_rng(22).random(685) < 0.25
    dq = torch.from_numpy(qf).to(dev)
    dex = torch.from_numpy(R.words_of(exclude).view(np.int64)).to(dev)
    dk = torch.full((40, topk), -6148914691236517206, dtype=torch.int64, device=dev)
    ds = torch.full((40, topk), float(SCORE_SENTINEL), dtype=torch.float32, device=dev)
    dc = torch.zeros((40,), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx = se.create_context()
    thr = -300.0
    assert se.search_fp32_dev(dq.data_ptr(), 100, 40, topk, refine, nprobe, NO_CUT, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx,
                              threshold=thr, d_exclude=dex.data_ptr(), stream=stream.cuda_stream) == 0
    stream.synchronize()                                                    # (the read-back waits for the context's stream, not a caller's)
    cand = se.last_candidates(ctx, 40, kc)
    gk, gs, gc = dk.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dc.cpu().numpy().view(np.uint32)
    F.check_stage1(*cand, cent, offs, rows, qbits, kc, nprobe, NO_CUT, exclude, what="dev")
    F.check_stage2_exact(gk, gs, gc, cand[0], cand[2], frows, qf, F.IP, topk, thr, what="dev")
    beyond = np.arange(topk)[None, :] >= gc[:, None]
    assert np.all(gk[beyond] == np.uint64(0xaaaaaaaaaaaaaaaa)) and np.all(gs[beyond] == SCORE_SENTINEL)
    assert 0 < gc.sum() < 40 * topk                                         # (the radius cut something, not everything)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_no_output():
    from zvec_amd import _lib
    L = _lib.lib()
    fx = F.fp_index(np.random.default_rng(31), 100, R.RAGGED, True, nq=6)
    cent, offs, rows, frows, qf, qbits = fx
    se = _searcher(100)
    ctx = se.create_context()

    def refused(handle, code, topk=5, refine=4, nprobe=3, q=qf, dim=None):
        rc, k, s, c = _raw(handle, ctx, q, topk, refine, nprobe, dim=dim)
        assert rc == code, (rc, code)
        assert _untouched(k, s, c)

    refused(se, NO_INDEX_LOADED)
    assert se.attach_rows(frows[:0], F.L2) == NO_INDEX_LOADED
    assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 100, 0) == NO_INDEX_LOADED
    assert se.load(cent, offs, rows) == 0
    assert se.attach_rows(frows[:5], F.L2) == INVALID                       # (the Python layer: row count != the index's)
    refused(se, NO_READY)
    pos = np.arange(3, dtype=np.uint64)
    out = np.full((3, 100), SCORE_SENTINEL, np.float32)
    assert L.zvec_hip_bivf_get_rows(se._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), 3, _ptr(out)) == NO_READY and np.all(out == SCORE_SENTINEL)
    with pytest.raises(Exception):
        se.last_candidates(ctx, 6, 20)
    assert L.zvec_hip_bivf_last_candidates(se._h, ctx._h, 6, 20, None, None, None) == NO_READY
    # attach_rows: width, metric
    assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 96, 0) == MISMATCH
    assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 129, 0) == MISMATCH
    assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 0, 0) == INVALID
    for metric in (2, 3, 7):                                                # cosine, Hamming, nonsense
        assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 100, metric) == UNSUPPORTED
    assert se.rows_info() == (0, 0, 0)
    assert se.attach_rows(frows, F.L2) == 0
    assert L.zvec_hip_bivf_attach_rows(se._h, _ptr(frows), 100, 2) == UNSUPPORTED and se.rows_info() == (100, 0, 685 * 400)
    # search
    refused(se, INVALID, topk=0)
    refused(se, INVALID, refine=0)
    refused(se, INVALID, nprobe=0)
    refused(se, UNSUPPORTED, topk=129)
    refused(se, MISMATCH, q=np.ascontiguousarray(qf[:, :99]))
    refused(se, MISMATCH, q=np.ascontiguousarray(qf[:, :96]))
    # get_rows beyond the count
    bad = np.array([0, 685], np.uint64)
    assert L.zvec_hip_bivf_get_rows(se._h, bad.ctypes.data_as(C.POINTER(C.c_uint64)), 2, _ptr(out)) == NO_EXIST and np.all(out == SCORE_SENTINEL)
    # a DT_BINARY64 handle, and build_fp32's own refusals leave a handle as it was
    b64 = _searcher(128, "binary64")
    assert b64.build_fp32(frows, 3) == MISMATCH and b64.info() == (0, 0)
    assert L.zvec_hip_bivf_attach_rows(b64._h, _ptr(frows), 100, 0) == MISMATCH
    before = _export_bytes(se)
    assert se.build_fp32(frows[:, :64], 3) == MISMATCH                      # 64 bits wanted, the handle has 128
    assert se.build_fp32(frows, 3, "Cosine") == UNSUPPORTED
    assert se.build_fp32(frows, 0) == INVALID and se.build_fp32(frows[:2], 3) == INVALID
    assert _export_bytes(se) == before and se.rows_info() == (100, 0, 685 * 400)
    _check(se, fx, F.L2, 5, 4, 3, True, what="after the refusals")
    # dim above the kernel's cap: rows that wide can be attached, the search refuses them
    wide_dim = 16128 + 32
    wide = _searcher(wide_dim)
    wb = np.zeros((2, wide_dim // 32), np.uint32)
    assert wide.load(wb[:1], np.array([0, 2], np.uint64), wb) == 0
    wf = np.ones((2, wide_dim), np.float32)
    assert wide.attach_rows(wf, F.L2) == 0
    refused(wide, UNSUPPORTED, q=wf)
    at_cap = _searcher(16128)
    cb = np.zeros((2, 16128 // 32), np.uint32)
    assert at_cap.load(cb[:1], np.array([0, 2], np.uint64), cb) == 0
    cf = np.zeros((2, 16128), np.float32)
    cf[1, ::2] = 1.0
    assert at_cap.attach_rows(cf, F.L2) == 0
    rc, k, s, c = _raw(at_cap, at_cap.create_context(), cf, 2, 1, 1)
    assert rc == 0 and np.array_equal(c, [2, 2]) and np.array_equal(k, [[0, 1], [1, 0]]) and np.array_equal(s, [[0, 8064], [0, 8064]])


def test_plain_search_on_a_handle_with_rows_answers_as_before():
    fx = F.fp_index(np.random.default_rng(41), 96, R.RAGGED, True)
    cent, offs, rows, frows, qf, qbits = fx
    bare = _searcher(96)
    assert bare.load(cent, offs, rows) == 0
    se = _attached(cent, offs, rows, frows, 96, F.L2)
    ctx = se.create_context()
    _check(se, fx, F.L2, 5, 4, 3, True, ctx=ctx)
    out = []
    for s, c in ((se, ctx), (bare, bare.create_context())):
        c.set_topk(10)
        assert s.search_impl(qbits, 40, c, nprobe=3, max_scan=NO_CUT) == 0
        out.append((c.keys.copy(), c.scores.copy(), c.counts.copy()))
    _, _, _, adm = R.model(cent, offs, qbits, 3, NO_CUT)
    check_hamming_lists(*out[0], hamming_reference(rows, qbits), 10, admissible=adm)
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
    from zvec_amd import _lib
    assert _lib.lib().zvec_hip_bivf_last_candidates(se._h, ctx._h, 40, 20, None, None, None) == NO_READY    # (the last search was plain)


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hamming_ivf_rerank")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "hamming_ivf_rerank.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert out.stdout.decode().count("query") == 4
