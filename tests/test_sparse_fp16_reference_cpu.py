"""The fp16 cases of tests/sparse_fp16_ref.py before the GPU is asked: the checker of tests/sparse_ref.py accepts a plain numpy fp32
evaluation of the integer data (bit for bit the fp64 reference), refuses an evaluation that keeps its sums in float16, the rounded
cases are deterministic and read-only, and the fp16 LDS size of the scan fits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_fp16_ref as H  # noqa: E402
import sparse_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nq", [1, 64, 65])
@pytest.mark.parametrize("k", [10, 200])
def test_checker_accepts_numpy_fp32_on_the_integer_data(nq, k):
    rows, queries, ref, A, m = H.make_integer_case(nq)
    n = H.INT_N
    assert len(rows[0]) == n and set(rows[0].tolist()) == set(H.INT_LENGTHS) and np.abs(rows[2]).max() == 8
    key_of_row, adm = np.arange(n, dtype=np.uint64), np.ones(n, bool)
    keys, scores, counts = R.lists_from_scores(R.fp32_scores(rows, queries), k, None, adm, key_of_row)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, adm, key_of_row)
    H.assert_exact(keys, scores, counts, ref, key_of_row)
    assert scores[0, 0] == -262144.0               # query 0 and row 0 hold all 4096 indices with value 8


@pytest.mark.parametrize("nq", [1, 65])
def test_checker_rejects_sums_kept_in_float16(nq):
    rows, queries, ref, A, m = H.make_integer_case(nq)
    n = H.INT_N
    key_of_row, adm = np.arange(n, dtype=np.uint64), np.ones(n, bool)
    s16 = H.half_accumulated_scores(rows, queries)
    assert not np.array_equal(s16, ref.astype(np.float32))
    for k in (10, 200):
        keys, scores, counts = R.lists_from_scores(s16, k, None, adm, key_of_row)
        with pytest.raises(AssertionError):
            R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, adm, key_of_row)
        with pytest.raises(AssertionError):
            H.assert_exact(keys, scores, counts, ref, key_of_row)


def test_rounded_cases_are_halves_deterministic_and_read_only():
    H.make_case.cache_clear()
    H.make_integer_case.cache_clear()
    first = H.make_case(65, 64, 100000, True), H.make_integer_case(65)
    H.make_case.cache_clear()
    H.make_integer_case.cache_clear()
    again = H.make_case(65, 64, 100000, True), H.make_integer_case(65)
    for a, b in zip(first, again):
        for u, v in zip(a[0] + a[1] + a[2:], b[0] + b[1] + b[2:]):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert H.make_case(65, 64, 100000, True) is again[0] and first[0][2] is not again[0][2]
    rows, queries, ref, A, m = again[0]
    plain = R.make_case(65, 64, 100000, True)
    for got, src in ((rows, plain[0]), (queries, plain[1])):
        assert got[0].tobytes() == src[0].tobytes() and got[1].tobytes() == src[1].tobytes()
        assert got[2].dtype == np.float32 and got[2].tobytes() == src[2].astype(np.float16).astype(np.float32).tobytes()
        assert H.halves(got)[2].dtype == np.float16
    assert ref.shape == (64, 65) and not np.array_equal(ref, plain[2])           # (the rounding is seen by the reference)
    for a in rows + queries + (ref, A, m):
        assert not a.flags.writeable
        with pytest.raises(ValueError):
            a[...] = 0
    with pytest.raises(AssertionError):
        H.halves(plain[0])                                                         # (fp32 values that are no halves)


def test_fp16_lds_size_fits():
    # k = 128 is the longest fused list (SPARSE_FUSED_MAX_K), 4096 elements the largest image (SPARSE_IMG_ELEMS)
    assert H.sparse_lds_bytes_fp16(4096, 128) == (128 * 128 + 4096) * 4 + 8192 + 16 < 96 * 1024
    assert H.sparse_lds_bytes_fp16(4096, 0) == 4096 * 6 + 16
    assert H.sparse_lds_bytes_fp16(3, 0) == 12 + 8 + 16                          # halves rounded up to whole words
    text = open(os.path.join(ROOT, "zvec_amd", "csrc", "zvk_sparse.hip.h")).read()
    assert "((size_t)2 * SPARSE_QB * k_lists + img_elems) * 4 + (((size_t)img_elems * width + 3) & ~(size_t)3) + 16" in text


def test_header_declares_the_typed_entries_and_binding_agrees():
    from zvec_amd import _lib
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    for name in ("create_typed", "dtype"):
        assert "zvec_hip_sparse_%s(" % name in text and "zvec_hip_sparse_" + name in _lib.SYMBOLS
    assert "#define ZVEC_HIP_ABI_VERSION 1" in text
    L = _lib.lib()
    import ctypes as C
    out = C.c_void_p(0x55)
    for bad in (_lib.DT_BINARY32, _lib.DT_BINARY64, 4, -1):
        assert L.zvec_hip_sparse_create_typed(bad, 0, C.byref(out)) == -12 and out.value == 0x55      # (before any device call)
    assert L.zvec_hip_sparse_create_typed(_lib.DT_FP16, 0, None) == -31
    assert L.zvec_hip_sparse_dtype(None, C.byref(C.c_int(0))) == -31
