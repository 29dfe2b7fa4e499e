"""CPU checks of the Hamming feature: the numpy reference against a pure-Python popcount, the list checker against lists that
are wrong in each way it must notice, the names and constants of the new data types and metric, the C example."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_matches_python_popcount():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 2**32, (50, 3), dtype=np.uint64).astype(np.uint32)      # 96 bits
    qs = rng.integers(0, 2**32, (7, 3), dtype=np.uint64).astype(np.uint32)
    ref = hamming_reference(base, qs, chunk=16)
    assert ref.shape == (7, 50) and ref.dtype == np.int64
    for q in range(7):
        for i in range(50):
            assert ref[q, i] == sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(base[i], qs[q]))
    # the same bits as uint64 words give the same distances
    assert np.array_equal(hamming_reference(np.ascontiguousarray(base[:, :2]).view(np.uint64), np.ascontiguousarray(qs[:, :2]).view(np.uint64)),
                          hamming_reference(base[:, :2], qs[:, :2]))


def _good_lists(ref, k, admissible=None):
    nq, n = ref.shape
    keys = np.full((nq, k), 2**64 - 1, np.uint64)
    scores = np.full((nq, k), np.inf, np.float32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        rows = [r for r in np.argsort(ref[q], kind="stable") if admissible is None or admissible[r]][:k]
        counts[q] = len(rows)
        keys[q, :len(rows)] = rows
        scores[q, :len(rows)] = ref[q, rows]
    return keys, scores, counts


def test_checker_rejects_wrong_lists():
    rng = np.random.default_rng(4)
    base = rng.integers(0, 2**32, (200, 3), dtype=np.uint64).astype(np.uint32)
    qs = rng.integers(0, 2**32, (4, 3), dtype=np.uint64).astype(np.uint32)
    ref = hamming_reference(base, qs)
    k = 10
    adm = np.ones(200, bool)
    adm[::7] = False
    keys, scores, counts = _good_lists(ref, k, adm)
    check_hamming_lists(keys, scores, counts, ref, k, admissible=adm)
    # equal scores may come in any order: swapping two tied entries (if any) still passes
    for q in range(4):
        for j in range(k - 1):
            if scores[q, j] == scores[q, j + 1]:
                k2 = keys.copy()
                k2[q, j], k2[q, j + 1] = keys[q, j + 1], keys[q, j]
                check_hamming_lists(k2, scores, counts, ref, k, admissible=adm)

    def rejected(kk, ss, cc, **kw):
        with pytest.raises(AssertionError):
            check_hamming_lists(kk, ss, cc, ref, k, admissible=adm, **kw)

    s2 = scores.copy()
    s2[1, 3] += 1                                   # one score off by 1
    rejected(keys, s2, counts)
    q, j = next((q, j) for q in range(4) for j in range(k - 1) if scores[q, j] != scores[q, j + 1])
    k2 = keys.copy()
    k2[q, j], k2[q, j + 1] = keys[q, j + 1], keys[q, j]        # key / score pairing swapped between two unequal scores
    rejected(k2, scores, counts)
    # a missing strictly-better row: the best row is replaced by another row of the LAST score's value (scores then shift)
    order = [r for r in np.argsort(ref[0], kind="stable") if adm[r]]
    rows = order[1:k + 1]
    k3, s3 = keys.copy(), scores.copy()
    k3[0], s3[0] = rows, ref[0, rows]
    assert ref[0, order[0]] < ref[0, rows[-1]]
    rejected(k3, s3, counts)
    k4 = keys.copy()
    k4[2, 5] = k4[2, 4]                             # a duplicate
    rejected(k4, scores, counts)
    k5, s5 = keys.copy(), scores.copy()
    bad = int(np.nonzero(~adm)[0][0])               # an excluded key, with its true score, placed where it sorts
    k5[3, 0], s5[3, 0] = bad, ref[3, bad]
    s5[3] = np.sort(s5[3])
    rejected(k5, s5, counts)
    c6 = counts.copy()
    c6[0] -= 1                                      # a short count
    rejected(keys, scores, c6)
    rejected(keys, scores, counts, threshold=float(scores[0, 2]))    # a radius the list ignores


def test_names_resolve_and_unknown_dtype_raises():
    from zvec_amd import index as I
    assert I.metric_from_name("Hamming") == I.METRIC_HAMMING == 3
    assert I._dtype_of("binary32") == (I.DT_BINARY32, np.uint32)
    assert I._dtype_of("binary64") == (I.DT_BINARY64, np.uint64)
    assert I._dtype_of(np.uint32) == (I.DT_BINARY32, np.uint32)
    assert I._dtype_of(np.uint64) == (I.DT_BINARY64, np.uint64)
    assert I._dtype_of("fp32") == (I.DT_FP32, np.float32) and I._dtype_of("fp16") == (I.DT_FP16, np.float16)
    assert I._dtype_of(np.float16) == (I.DT_FP16, np.float16) and I._dtype_of(I.DT_FP16) == (I.DT_FP16, np.float16)
    for bogus in ("int8", "binary", None, 7, np.int8):
        with pytest.raises(ValueError):
            I._dtype_of(bogus)


def test_header_declares_the_constants_and_binding_agrees():
    from zvec_amd import _lib
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ZVEC_HIP_(?:DT|METRIC)_[A-Z0-9]+)\s*=\s*(\d+)", text)}
    assert values["ZVEC_HIP_DT_BINARY32"] == 2 == _lib.DT_BINARY32
    assert values["ZVEC_HIP_DT_BINARY64"] == 3 == _lib.DT_BINARY64
    assert values["ZVEC_HIP_METRIC_HAMMING"] == 3 == _lib.METRIC_HAMMING
    assert (values["ZVEC_HIP_DT_FP32"], values["ZVEC_HIP_DT_FP16"]) == (_lib.DT_FP32, _lib.DT_FP16) == (0, 1)
    assert (values["ZVEC_HIP_METRIC_L2"], values["ZVEC_HIP_METRIC_IP"], values["ZVEC_HIP_METRIC_COSINE"]) == (0, 1, 2)


def test_c_example_compiles_as_c99():
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hamming_search")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "hamming_search.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        assert os.path.exists(exe)
