"""tests/hamming_ivf_fp32_ref.py on the CPU: the fixtures of tests/test_gpu_hamming_ivf_fp32.py meet the preconditions that keep a
GPU test from passing vacuously, and each checker refuses a hand-made wrong answer.  Nothing here touches the GPU."""
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
from hamming_ref import hamming_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK, REFINE = 5, 4
KC = F.kc_of(TOPK, REFINE)


def _answer(pos, cnt, frows, qf, metric, topk, threshold=None):
    """stage2_exact as output arrays"""
    keys = np.full((qf.shape[0], topk), 0xdeadbeef, np.uint64)
    scores = np.full((qf.shape[0], topk), -1.0, np.float32)
    counts = np.zeros(qf.shape[0], np.uint32)
    for i, (k, s) in enumerate(F.stage2_exact(pos, cnt, frows, qf, metric, topk, threshold)):
        keys[i, :k.size], scores[i, :k.size], counts[i] = k, s, k.size
    return keys, scores, counts


def test_scores_and_band_by_hand():
    rows = np.array([[1, -2, 3], [0, 0, 0]], np.float32)
    q = np.array([[2, 2, -1]], np.float32)
    assert np.array_equal(F.fp64_scores(rows, q, F.L2), [[1 + 16 + 16, 4 + 4 + 1]])
    assert np.array_equal(F.fp64_scores(rows, q, F.IP), [[-(2 - 4 - 3), 0]])
    assert np.array_equal(F.band(rows, q, F.L2), 5 * 2.0 ** -23 * np.array([[33.0, 9.0]]))
    assert np.array_equal(F.band(rows, q, F.IP), 5 * 2.0 ** -23 * np.array([[9.0, 0.0]]))
    assert F.kc_of(5, 4) == 20 and F.kc_of(40, 8) == 128 and F.kc_of(128, 1) == 128 and F.dim_bits(100) == 128 and F.dim_bits(96) == 96
    # the band is more than twice the standard bound gamma_(dim + 2) of an fp32 sum, for every dim in use
    for dim in (33, 96, 100, 768):
        u = 2.0 ** -24
        assert (dim + 2) * 2.0 ** -23 > 2 * ((dim + 2) * u / (1 - (dim + 2) * u)) * 0.999


@pytest.mark.parametrize("dim", [96, 100, 33])
@pytest.mark.parametrize("integer", [True, False])
def test_attach_fixture(dim, integer):
    cent, offs, rows, frows, qf, qbits = F.fp_index(np.random.default_rng(dim), dim, R.RAGGED, integer)
    assert qf.shape == (40, dim) and frows.shape == (685, dim) and rows.shape[1] == F.dim_bits(dim) // 32
    assert np.array_equal(binary_encode_reference(qf), qbits) and np.array_equal(binary_encode_reference(frows), rows)
    if integer:
        assert np.abs(frows).max() <= 8 and np.abs(qf).max() <= 8 and np.array_equal(frows, np.round(frows))
        assert dim * 16 * 16 < 2 ** 24                                    # every partial sum is an integer below 2^24
    # ties really straddle the kc-th place of stage 1 for some query, at nprobe = nlist
    ref = np.sort(hamming_reference(rows, qbits), axis=1)
    assert np.any(ref[:, KC - 1] == ref[:, KC])
    # at most 1 query in 20 is ambiguous for the fp64 reference itself
    for nprobe in (1, 3, 6):
        pos, cnt = F.model_candidates(cent, offs, rows, qbits, KC, nprobe)
        for metric in (F.L2, F.IP):
            amb = 0
            for i in range(40):
                c = pos[i, :cnt[i]].astype(np.int64)
                amb += F.ambiguous_cut(F.fp64_scores(frows[c], qf[i:i + 1], metric)[0], F.band(frows[c], qf[i:i + 1], metric)[0], TOPK)
            if not integer:
                assert amb <= 2, (nprobe, metric, amb)


def test_short_list_fixture():
    cent, offs, rows, frows, qf, qbits, lst = F.short_list(np.random.default_rng(5))
    assert int(offs[lst + 1] - offs[lst]) == 3 < TOPK
    assert np.all(R.probe_order(cent, qbits, 1)[:, 0] == lst)
    pos, cnt = F.model_candidates(cent, offs, rows, qbits, KC, 1)
    assert np.all(cnt == 3)


def test_two_slice_fixture():
    cent, offs, rows, frows, qf, qbits, nprobe, topk, refine, cap = F.two_slices(np.random.default_rng(6))
    assert R.min_slices(qbits.shape[0], nprobe, F.kc_of(topk, refine), cap) >= 2
    assert cap >= 1024                                                    # the option's lower limit


def test_max_scan_fixture():
    cent, offs, rows, frows, qf, qbits, nprobe, length = F.max_scan_case(np.random.default_rng(4))
    assert length > 0 and np.array_equal(binary_encode_reference(qf), qbits)
    _, cnt, _, _ = R.model(cent, offs, qbits, nprobe, length)
    assert cnt[0] == 1 and R.model(cent, offs, qbits, nprobe, length + 1)[1][0] >= 2       # the cut really moves with the count


def _integer_case():
    cent, offs, rows, frows, qf, qbits = F.fp_index(np.random.default_rng(96), 96, R.RAGGED, True)
    pos, cnt = F.model_candidates(cent, offs, rows, qbits, KC, 3)
    return cent, offs, rows, frows, qf, qbits, pos, cnt


def test_stage1_checker_refuses_wrong_candidates():
    cent, offs, rows, frows, qf, qbits, pos, cnt = _integer_case()
    ham = np.take_along_axis(hamming_reference(rows, qbits), np.minimum(pos, rows.shape[0] - 1).astype(np.int64), axis=1).astype(np.float32)
    F.check_stage1(pos, ham, cnt, cent, offs, rows, qbits, KC, 3)
    # a candidate outside the probed set
    _, _, _, adm = R.model(cent, offs, qbits, 3, 0xffffffff)
    bad = pos.copy()
    bad[0, 0] = np.nonzero(~adm[0])[0][0]
    with pytest.raises(AssertionError):
        F.check_stage1(bad, ham, cnt, cent, offs, rows, qbits, KC, 3)
    # a swapped pair of different scores: no longer ascending
    q = next(i for i in range(40) if ham[i, 0] != ham[i, cnt[i] - 1])
    bad, bads = pos.copy(), ham.copy()
    bad[q, [0, cnt[q] - 1]] = bad[q, [cnt[q] - 1, 0]]
    bads[q, [0, cnt[q] - 1]] = bads[q, [cnt[q] - 1, 0]]
    with pytest.raises(AssertionError):
        F.check_stage1(bad, bads, cnt, cent, offs, rows, qbits, KC, 3)
    # a query left short
    short = cnt.copy()
    short[1] -= 1
    with pytest.raises(AssertionError):
        F.check_stage1(pos, ham, short, cent, offs, rows, qbits, KC, 3)


@pytest.mark.parametrize("metric", [F.L2, F.IP])
def test_stage2_exact_checker_refuses_wrong_answers(metric):
    cent, offs, rows, frows, qf, qbits, pos, cnt = _integer_case()
    keys, scores, counts = _answer(pos, cnt, frows, qf, metric, TOPK)
    F.check_stage2_exact(keys, scores, counts, pos, cnt, frows, qf, metric, TOPK)
    assert F.check_stage2_real(keys, scores, counts, pos, cnt, frows, qf, metric, TOPK) <= 40
    # a swapped pair
    bad = keys.copy()
    bad[0, [0, 1]] = bad[0, [1, 0]]
    with pytest.raises(AssertionError):
        F.check_stage2_exact(bad, scores, counts, pos, cnt, frows, qf, metric, TOPK)
    # a candidate outside the set
    outside = np.setdiff1d(np.arange(rows.shape[0]), pos[0, :cnt[0]])[0]
    bad = keys.copy()
    bad[0, 0] = outside
    with pytest.raises(AssertionError):
        F.check_stage2_exact(bad, scores, counts, pos, cnt, frows, qf, metric, TOPK)
    with pytest.raises(AssertionError):
        F.check_stage2_real(bad, scores, counts, pos, cnt, frows, qf, metric, TOPK)
    # a score one ulp off
    bads = scores.copy()
    bads[2, 1] = np.nextafter(bads[2, 1], np.float32(np.inf))
    with pytest.raises(AssertionError):
        F.check_stage2_exact(keys, bads, counts, pos, cnt, frows, qf, metric, TOPK)
    # the radius: every score beyond it drops, a count that ignores it is refused
    thr = float(np.median(scores[:, 2]))
    tk, ts, tc = _answer(pos, cnt, frows, qf, metric, TOPK, thr)
    assert tc.min() < TOPK and np.all(ts[np.arange(TOPK)[None, :] < tc[:, None]] <= thr)
    F.check_stage2_exact(tk, ts, tc, pos, cnt, frows, qf, metric, TOPK, thr)
    with pytest.raises(AssertionError):
        F.check_stage2_exact(keys, scores, counts, pos, cnt, frows, qf, metric, TOPK, thr)


@pytest.mark.parametrize("metric", [F.L2, F.IP])
def test_stage2_real_checker_refuses_wrong_answers(metric):
    cent, offs, rows, frows, qf, qbits = F.fp_index(np.random.default_rng(100), 100, R.RAGGED, False)
    pos, cnt = F.model_candidates(cent, offs, rows, qbits, KC, 3)
    keys = np.zeros((40, TOPK), np.uint64)
    scores = np.zeros((40, TOPK), np.float32)
    counts = np.zeros(40, np.uint32)
    for i in range(40):
        c = pos[i, :cnt[i]].astype(np.int64)
        s = F.fp64_scores(frows[c], qf[i:i + 1], metric)[0]
        o = np.argsort(s, kind="stable")[:TOPK]
        keys[i, :o.size], scores[i, :o.size], counts[i] = c[o], s[o].astype(np.float32), o.size
    assert F.check_stage2_real(keys, scores, counts, pos, cnt, frows, qf, metric, TOPK) <= 2
    q = next(i for i in range(40) if cnt[i] > TOPK and not F.ambiguous_cut(
        F.fp64_scores(frows[pos[i, :cnt[i]].astype(np.int64)], qf[i:i + 1], metric)[0],
        F.band(frows[pos[i, :cnt[i]].astype(np.int64)], qf[i:i + 1], metric)[0], TOPK))
    # the worst candidate in the best one's place: wrong set, and its score is out of the band
    c = pos[q, :cnt[q]].astype(np.int64)
    worst = c[np.argmax(F.fp64_scores(frows[c], qf[q:q + 1], metric)[0])]
    bad = keys.copy()
    bad[q, 0] = worst
    with pytest.raises(AssertionError):
        F.check_stage2_real(bad, scores, counts, pos, cnt, frows, qf, metric, TOPK)
    # a score beyond the band
    bads = scores.copy()
    bads[q, 0] += np.float32(4 * F.band(frows[[int(keys[q, 0])]], qf[q:q + 1], metric)[0, 0] + 1e-6)
    with pytest.raises(AssertionError):
        F.check_stage2_real(keys, bads, counts, pos, cnt, frows, qf, metric, TOPK)


def test_c_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hamming_ivf_rerank")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "hamming_ivf_rerank.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-lm", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        assert os.path.exists(exe)
