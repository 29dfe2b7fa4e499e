"""What the fixtures of tests/hnsw_f16_ref.py must show before the GPU tests lean on them (no GPU): every array is made of binary16
values, the exact fixtures keep the bound that makes the fp64 models exact, the hand-made graphs in use are named, the planted
subnormals, -0.0 and largest half are really there, and the half conversion of examples/hnsw_fp16.c agrees with numpy."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_f16_ref as F  # noqa: E402
import hnsw_ref as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _round_trip(a16):
    assert a16.dtype == np.float16
    back = F.widen(a16).astype(np.float16)
    assert np.array_equal(back.view(np.uint16), a16.view(np.uint16))
    assert np.isfinite(F.widen(a16)).all()


def test_every_fixture_array_survives_the_round_trip():
    for dim in F.EXACT_DIMS:
        t = F.exact_twin(dim)
        _round_trip(t.rows16)
        _round_trip(t.queries16)
        assert np.array_equal(F.widen(t.rows16), t.graph.rows)             # the model's rows ARE the widened halves
    _round_trip(F.HAND_QUERIES)
    for dim in (5, 64):
        _round_trip(F.build_rows(300, dim)[0])
    for dim in F.REAL_DIMS:
        _round_trip(F.real_rows(F.REAL_N, dim, 1))
        _round_trip(F.real_rows(F.REAL_Q, dim, 2))
    t = F.planted_twin()
    _round_trip(t.rows16)
    _round_trip(t.queries16)
    assert np.array_equal(F.widen(t.rows16).view(np.uint32), t.graph.rows.view(np.uint32))


def test_exact_fixtures_keep_the_bound_of_exact_rows():
    """integers in [-8, 8], dim <= 128: a squared distance is at most 128 * 16^2 = 2^15, every partial sum an integer below 2^24"""
    arrays = [a for dim in F.EXACT_DIMS for a in F.exact_twin(dim)[:2]] + [F.build_rows(300, dim)[0] for dim in (5, 64)]
    for a in arrays:
        w = F.widen(a)
        assert a.shape[1] <= 128 and np.array_equal(w, np.round(w)) and np.abs(w).max() <= 8
    assert max(F.EXACT_DIMS) * 16 ** 2 < 2 ** 24


def test_the_hand_made_graphs_in_use():
    used = F.usable_hand_made()
    print("hand-made graphs with binary16 rows:", ", ".join(used))
    assert len(used) > 0
    assert set(used) == {"chain", "star", "two_components", "with_empty_lists", "bare_upper", "single", "duplicate_ids", "tie_ring"}
    for name, f in used.items():
        g = f()
        assert g.rows.shape[1] == F.HAND_QUERIES.shape[1]
        _round_trip(g.rows.astype(np.float16))
        assert np.array_equal(F.widen(g.rows.astype(np.float16)), g.rows), name
    assert not F.is_half(np.array([[0.1]], np.float32)) and not F.is_half(np.array([[2049.0]], np.float32))      # (the filter filters)


def test_the_plants_are_present():
    t = F.planted_twin()
    bits = t.rows16.view(np.uint16)
    sub = ((bits & 0x7c00) == 0) & ((bits & 0x03ff) != 0)
    assert int(sub.sum()) >= 36 + 20                                       # "a few dozen" across the rows, and most of PLANT_ROW
    assert int(sub[np.arange(F.REAL_N) != F.PLANT_ROW].sum()) >= 30
    assert int((bits == 0x8000).sum()) >= 10                               # -0.0
    assert bits[F.PLANT_MAX_ROW, 5] == 0x7bff and float(t.rows16[F.PLANT_MAX_ROW, 5]) == F.HALF_MAX
    assert int((bits == 0x7bff).sum()) == 1
    row = bits[F.PLANT_ROW]
    assert ((row & 0x7c00) == 0).all() and (row == 0x8000).any() and ((row & 0x03ff) != 0).sum() > 40
    q = t.queries16.view(np.uint16)[F.PLANT_QUERY]
    assert ((q & 0x7c00) == 0).all() and (q == 0x8000).any() and ((q & 0x03ff) != 0).sum() > 40
    # a flush of subnormals to zero anywhere would show: the all-subnormal query has non-zero scores against ordinary rows
    w = F.widen(t.queries16[F.PLANT_QUERY]).astype(np.float64)
    assert (np.abs(t.graph.rows[:10].astype(np.float64) @ w) > 0).all()
    # and the largest half squared stays far inside fp32
    assert F.HALF_MAX ** 2 * 4 < np.finfo(np.float32).max


def test_the_spill_case_spills():
    """every query's candidate set passes the 1024 words the kernel holds in LDS, by a margin fp32 rounding cannot close"""
    t = F.spill_twin()
    _round_trip(t.rows16)
    _round_trip(t.queries16)
    peaks = [H.search_model(t.graph, F.widen(q), 10, 512, exclude=F.spill_exclude()).c_peak for q in t.queries16]
    print("most candidates alive:", peaks)
    assert min(peaks) > H.C_LDS + 50


def test_the_examples_half_conversion_agrees_with_numpy():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "half.so")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-DHNSW_FP16_NO_MAIN",
                               "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "examples", "hnsw_fp16.c")])
        L = C.CDLL(so)
        L.half_of_float.restype, L.half_of_float.argtypes = C.c_uint16, [C.c_float]
        L.float_of_half.restype, L.float_of_half.argtypes = C.c_float, [C.c_uint16]
        own = (np.arange(-32, 33) * 0.25).astype(np.float32)              # the example's own data: -8 .. 8 in steps of 1/4
        rng = np.random.default_rng(1)
        more = np.concatenate([rng.standard_normal(2000).astype(np.float32), (rng.standard_normal(500) * 1e-6).astype(np.float32),
                               (np.arange(0, 2048) * F.SUB / 2).astype(np.float32),      # subnormals and the ties between them
                               np.array([0.0, -0.0, 65504.0, -65504.0, 65519.0, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -14,
                                         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2047.5, 1e-30], np.float32)])
        for v in np.concatenate([own, more]):
            want = np.float32(v).astype(np.float16)
            got = L.half_of_float(float(v))
            assert got == int(want.view(np.uint16)), (float(v), got, int(want.view(np.uint16)))
        for v in own:
            assert L.float_of_half(L.half_of_float(float(v))) == float(v)
        every = np.arange(0, 0x7c00, dtype=np.uint16)                      # every finite non-negative half, and its negative
        for bits in np.concatenate([every[::7], every[:1100], every[-5:], every[::11] | np.uint16(0x8000)]):
            want = np.array([bits], np.uint16).view(np.float16).astype(np.float32)[0]
            got = np.float32(L.float_of_half(int(bits)))
            assert got.view(np.uint32) == want.view(np.uint32), int(bits)
