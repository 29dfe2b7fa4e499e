"""The model of the Hamming IVF index (tests/hamming_ivf_ref.py) pinned by hand, every fixture of tests/test_gpu_hamming_ivf.py held to
the precondition that keeps its GPU test from passing vacuously, and the new entry points declared, bound and exported.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ivf_ref as R  # noqa: E402
from hamming_ref import hamming_reference  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["create", "destroy", "load", "build", "build_dev", "info", "export", "get_vectors", "search", "search_dev", "last_probes"]


def test_hand_computed_case():
    """3 centroids, 6 rows of 32 bits"""
    cent = np.array([[0x00000000], [0x0000000f], [0xffffffff]], np.uint32)
    rows = np.array([[0x00000001], [0x00000003], [0x0000001f], [0x0000000f], [0xfffffffe], [0x7fffffff]], np.uint32)
    offs = np.array([0, 2, 4, 6], np.uint64)
    q = np.array([[0x00000003], [0xffffffff]], np.uint32)
    # distances of the queries to the centroids: (2, 2, 30) and (32, 28, 0); query 0 ties centroids 0 and 1: the lower index first
    assert np.array_equal(hamming_reference(cent, q), [[2, 2, 30], [32, 28, 0]])
    assert np.array_equal(R.probe_order(cent, q, 2), [[0, 1], [2, 1]])
    assert np.array_equal(R.probe_order(cent, q, 1), [[0], [2]])
    assert np.array_equal(R.probe_order(cent, q, 7), [[0, 1, 2], [2, 1, 0]])
    # the cut: a list is probed while the rows before it are fewer than max_scan
    order = R.probe_order(cent, q, 3)
    for max_scan, cnt, scanned in ((0, 0, 0), (1, 1, 2), (2, 1, 2), (3, 2, 4), (4, 2, 4), (5, 3, 6), (100, 3, 6)):
        c, s = R.max_scan_cut(order, offs, max_scan)
        assert c.tolist() == [cnt, cnt] and s.tolist() == [scanned, scanned], max_scan
    _, cnt, _, adm = R.model(cent, offs, q, 2, 3)
    assert adm.tolist() == [[True, True, True, True, False, False], [False, False, True, True, True, True]]
    assert R.admissible(order[:, :1], np.array([1, 1]), offs, exclude=np.array([1, 0, 0, 0, 0, 1], bool)).tolist() == \
        [[False, True, False, False, False, False], [False, False, False, False, True, False]]
    # labels: row 1 (0x3) is 2 from centroid 0 and 2 from centroid 1: centroid 0
    lab = R.labels(cent, rows)
    assert lab.tolist() == [0, 0, 1, 1, 2, 2]
    # majority: list 0 = {0x1, 0x3}: bit 0 has 2 ones > 1, bit 1 has 1 one, not > 1; list 1 = {0x1f, 0x0f}: bits 0-3; list 2: bits 1-30
    assert R.majority_step(cent, rows, lab).tolist() == [[0x00000001], [0x0000000f], [0x7ffffffe]]
    # three members each, ones > 1: {0x1, 0x3, 0x1f} -> bits 0-1; {0xf, 0xfffffffe, 0x7fffffff} -> bit 0 twice, bits 1-30 at least
    # twice, bit 31 once; the centroid without members keeps its bits
    lab3 = np.array([0, 0, 0, 2, 2, 2])
    assert R.majority_step(cent, rows, lab3).tolist() == [[0x00000003], [0x0000000f], [0x7fffffff]]


def test_initial_rows_are_distinct_and_seeded():
    for n, nlist, seed in ((6, 6, 1), (1000, 70, 20260320), (70, 69, 2)):
        a = R.initial_rows(n, nlist, seed)
        assert len(set(a.tolist())) == nlist and a.min() >= 0 and a.max() < n
        assert np.array_equal(a, R.initial_rows(n, nlist, seed))
    assert not np.array_equal(R.initial_rows(1000, 70, 1), R.initial_rows(1000, 70, 2))
    # splitmix64(seed = 0): the first draw is 0xe220a8397b1dcdaf
    assert R.initial_rows(1 << 63, 1, 0)[0] == 0xe220a8397b1dcdaf % (1 << 63)


def test_fixture_ragged_lists():
    cent, offs, rows = R.index_of(np.random.default_rng(1), 96, R.RAGGED)
    lens = np.diff(offs.astype(np.int64))
    assert lens.tolist() == [0, 1, 127, 128, 129, 300] and rows.shape == (685, 3)
    starts, ends = offs[:-1].astype(np.int64), offs[1:].astype(np.int64)
    assert np.any(starts[lens > 0] % 128 != 0) and np.any(ends[lens > 0] % 128 != 0)       # lists start and end off the tile grid
    assert max((e - 1) // 128 - s // 128 + 1 for s, e in zip(starts, ends) if e > s) >= 3  # one list spans three tiles
    assert len(set((offs[1:][lens > 0] - 1) // 128) & set(offs[:-1][lens > 0] // 128)) > 0  # a tile shared by two lists


def test_fixture_duplicate_centroids_tie_at_the_probe_boundary():
    cent, offs, rows, q = R.duplicate_centroids(np.random.default_rng(2))
    d = hamming_reference(cent, q)
    assert np.array_equal(cent[1], cent[3])
    assert np.all(d[:, 1] == d[:, 3]) and np.all(d[:, 1] == d.min(axis=1))     # the pair is nearest, and tied
    assert np.all(R.probe_order(cent, q, 1)[:, 0] == 1)                        # so nprobe 1 cuts between them: the lower index
    assert np.array_equal(R.probe_order(cent, q, 2), np.tile([1, 3], (q.shape[0], 1)))


def test_fixture_crowded_lists():
    for nq in (33, 70):
        cent, offs, rows, q = R.crowded_lists(np.random.default_rng(3), nq)
        order, cnt, _, _ = R.model(cent, offs, q, 2, 1 << 30)
        per_list = np.bincount(np.concatenate([o[:c] for o, c in zip(order, cnt)]), minlength=2)
        assert np.all(per_list == nq) and nq > 32


def test_fixture_max_scan_cuts_before_nprobe():
    cent, offs, rows, q, nprobe, length = R.max_scan_case(np.random.default_rng(4))
    assert length > 0 and nprobe <= cent.shape[0]
    order = R.probe_order(cent, q, nprobe)
    cnt, scanned = R.max_scan_cut(order, offs, length)              # the first list's length: query 0 stops after it
    assert cnt[0] == 1 and scanned[0] == length and cnt[0] < nprobe
    cnt1, scanned1 = R.max_scan_cut(order, offs, length + 1)        # one more: the second list is probed as well
    assert cnt1[0] >= 2 and scanned1[0] > length
    assert len(set(cnt.tolist())) > 1                               # and the queries of the batch are cut at different ranks
    cnt0, scanned0 = R.max_scan_cut(order, offs, 0)
    assert not cnt0.any() and not scanned0.any()
    full, _ = R.max_scan_cut(order, offs, 1 << 30)
    assert np.all(full == nprobe)


def test_fixture_two_slices():
    cent, offs, rows, q, nprobe, k, cap = R.two_slices(np.random.default_rng(6))
    assert R.min_slices(q.shape[0], min(nprobe, cent.shape[0]), k, cap) >= 2
    assert R.min_slices(q.shape[0], min(nprobe, cent.shape[0]), k, 1 << 30) == 1
    assert 1024 <= cap <= 1 << 30                    # the option's range


def _declared():
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(zvec_hip_[a-z_0-9]+)\s*\(", text))


def test_entry_points_are_declared_bound_and_exported():
    from zvec_amd import _lib
    import zvec_amd
    names = ["zvec_hip_bivf_" + e for e in ENTRIES]
    decl = _declared()
    L = _lib.lib()
    for name in names:
        assert name in decl and name in _lib.SYMBOLS and hasattr(L, name), name
    for method in ("load", "build", "build_dev", "info", "export", "get_vectors_by_ids", "search_impl", "search_dev", "last_probes",
                   "set_nprobe"):
        assert callable(getattr(zvec_amd.HipHammingIVFSearcher, method)), method
    # null handles are refused before any device call; the slice cap is an option with a range
    assert L.zvec_hip_bivf_create(96, _lib.DT_BINARY32, 0, None) == -31
    assert L.zvec_hip_bivf_search(None, None, None, 1, 1, C.c_float(1.0), 1, 1, None, None, None, None) == -31
    assert L.zvec_hip_bivf_last_probes(None, None, 1, None, None, None) == -31
    assert L.zvec_hip_bivf_export(None, None, None, None) == -31
    v = C.c_int(0)
    assert L.zvec_hip_get_option(b"bivf_part_bytes", C.byref(v)) == 0 and v.value == 1 << 30
    assert L.zvec_hip_set_option(b"bivf_part_bytes", 1023) != 0 and L.zvec_hip_set_option(b"bivf_part_bytes", 4096) == 0
    assert L.zvec_hip_get_option(b"bivf_part_bytes", C.byref(v)) == 0 and v.value == 4096
    assert L.zvec_hip_set_option(b"bivf_part_bytes", 1 << 30) == 0
