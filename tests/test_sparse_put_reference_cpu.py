"""Add-with-id on the sparse index (zvec_hip_sparse_put), checked without a GPU: the Python model of tests/sparse_put_ref.py on
hand-written sequences, its store checker on stores that are wrong in one place, the three symbols in header, binding and library,
their NULL-handle answers, and examples/sparse_put.c as C99."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_put_ref as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["zvec_hip_sparse_put", "zvec_hip_sparse_holes", "zvec_hip_sparse_put_info"]
INVALID = -31


def _row(*pairs):
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.float32)


def _put(model, ids, rows, keys=None):
    M.apply_put(model, ids, *M.pack(rows, model.np_dtype), keys=keys)


def _lengths(model):
    return [int(r[0].size) for r in model.rows]


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_gap_is_padded_with_holes():
    m = M.PutModel("fp32")
    _put(m, [0, 1], [_row((3, 1.0)), _row((4, 2.0), (9, 3.0))])
    assert m.count() == 2 and m.holes == set() and m.keys == [0, 1]
    _put(m, [5], [_row((7, 4.0))])
    assert m.count() == 6 and m.holes == {2, 3, 4} and m.keys == [0, 1] + [M.INVALID_KEY] * 3 + [5]
    assert _lengths(m) == [1, 2, 0, 0, 0, 1] and m.elements() == 4
    assert m.hole_mask().tolist() == [False, False, True, True, True, False]


def test_a_written_hole_stops_being_a_hole():
    m = M.PutModel("fp32")
    _put(m, [3], [_row((1, 1.0))])
    assert m.holes == {0, 1, 2}
    _put(m, [1], [_row((2, 5.0), (6, 6.0))], keys=[77])
    assert m.holes == {0, 2} and m.keys[1] == 77 and _lengths(m) == [0, 2, 0, 1]
    _put(m, [0], [_row()])                                      # an empty row is a row, not a hole
    assert m.holes == {2} and m.keys[0] == 0 and _lengths(m)[0] == 0


def test_same_id_twice_keeps_the_later_row():
    m = M.PutModel("fp32")
    _put(m, [0, 1, 2], [_row((1, 1.0)), _row((1, 2.0)), _row((1, 3.0))])
    _put(m, [1, 1], [_row((5, 8.0), (6, 9.0)), _row((7, 10.0))], keys=[40, 41])
    assert m.rows[1][0].tolist() == [7] and m.rows[1][1].tolist() == [10.0] and m.keys[1] == 41
    # ... and call order decides inside one call: the pad of the first row is overwritten by the second
    _put(m, [5, 3], [_row((2, 1.0)), _row((3, 1.0))])
    assert m.holes == {4} and m.keys[3] == 3 and m.keys[5] == 5 and m.count() == 6


def test_overwrite_of_the_last_row():
    m = M.PutModel("fp16")
    _put(m, [0, 1], [_row((1, 1.0)), _row((2, 2.0))])
    _put(m, [1], [_row((2, 0.5), (3, 0.25), (4, 0.125))])
    assert m.count() == 2 and _lengths(m) == [1, 3] and m.elements() == 4
    assert m.rows[1][1].dtype == np.float16
    counts, idx, val = m.batch()
    assert counts.tolist() == [1, 3] and idx.tolist() == [1, 2, 3, 4] and val.dtype == np.float16


# ---- the checker ----------------------------------------------------------------------------------------------------------------
def _model_with_everything():
    rng = np.random.default_rng(5)
    m = M.PutModel("fp16")
    rows = [M.random_row(rng, c, 200, np.float16) for c in (4, 0, 9, 1)]
    _put(m, [0, 1, 2, 3], rows)
    _put(m, [6], [M.random_row(rng, 5, 200, np.float16)], keys=[1234])
    return m


def test_checker_accepts_the_model_itself():
    m = _model_with_everything()
    M.check_store(M.read_back_of_model(m), m)


def _spoil(what):
    m = _model_with_everything()
    got = M.read_back_of_model(m)
    if what == "index":
        got["rows"][2][0][3] += 1
    elif what == "value bit":
        M.raw(got["rows"][2][1])[5] ^= 1
    elif what == "key":
        got["keys"][6] = 1235
    elif what == "missed hole":
        got["hole"][4] = False
    elif what == "hole count":
        got["holes"] -= 1
    elif what == "element count":
        got["elements"] += 1
    elif what == "row count":
        got["count"] += 1
    return got, m


@pytest.mark.parametrize("what", ["index", "value bit", "key", "missed hole", "hole count", "element count", "row count"])
def test_checker_rejects_a_store_that_is_wrong_in_one_place(what):
    got, m = _spoil(what)
    with pytest.raises(AssertionError):
        M.check_store(got, m)


def test_values_are_compared_as_bits():
    m = M.PutModel("fp32")
    _put(m, [0], [_row((1, 0.0))])
    got = M.read_back_of_model(m)
    got["rows"][0][1][0] = np.float32(-0.0)                     # equal as numbers, another bit pattern
    with pytest.raises(AssertionError):
        M.check_store(got, m)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    from zvec_amd import _lib
    so = _lib.library_path()
    _lib.lib()
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(zvec_hip_[a-z_0-9]+)\s*\(", text))
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", so]).decode().splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name


def test_null_handle_is_an_invalid_argument():
    from zvec_amd import _lib
    L = _lib.lib()
    ids, counts = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    assert L.zvec_hip_sparse_put(None, C.c_void_p(ids.ctypes.data), C.c_void_p(counts.ctypes.data), None, None, 1, None) == INVALID
    n = C.c_uint64(7)
    assert L.zvec_hip_sparse_holes(None, C.byref(n)) == INVALID and n.value == 7
    route = C.c_int(9)
    assert L.zvec_hip_sparse_put_info(None, C.byref(route), None, None, None) == INVALID and route.value == 9


def test_c_example_compiles_as_c99():
    from zvec_amd import _lib
    _lib.lib()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sparse_put")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "sparse_put.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-lm",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        assert os.path.exists(exe)
