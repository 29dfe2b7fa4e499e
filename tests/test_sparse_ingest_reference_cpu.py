"""The numpy reference of tests/sparse_ingest_ref.py on hand-made cases: the kept-element rule, column order, append's CSR rules;
and the fp64 scorer of tests/sparse_ref.py on the CSR it produces against a dense evaluation of the same matrices."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ingest_ref as G  # noqa: E402
import sparse_ref as R  # noqa: E402


@pytest.mark.parametrize("dt", [np.float32, np.float16])
def test_kept_elements_and_their_order(dt):
    sub = np.array([1], np.uint16 if dt is np.float16 else np.uint32).view(dt)[0]      # the smallest subnormal
    m = np.zeros((5, 6), dt)
    m[0] = [0.0, 1.5, -0.0, sub, 0.0, -2.0]
    m[2, 0] = 3.0                                       # the first column alone
    m[3, 5] = -1.0                                      # the last column alone
    m[4] = [np.inf, np.nan, 0.0, -np.inf, 0.0, 1.0]
    counts, idx, val = G.dense_to_csr(m)
    assert counts.dtype == np.uint32 and idx.dtype == np.uint32 and val.dtype == dt
    assert counts.tolist() == [3, 0, 1, 1, 4]
    assert idx.tolist() == [1, 3, 5, 0, 5, 0, 1, 3, 5]
    want = np.array([1.5, sub, -2.0, 3.0, -1.0, np.inf, np.nan, -np.inf, 1.0], dt)
    assert G.raw(val).tobytes() == G.raw(want).tobytes()                # bit for bit: the subnormal and the NaN as they were
    assert G.check_csr(counts, idx, idx.size) == 0


def test_empty_shapes():
    for shape in [(0, 7), (3, 0)]:
        counts, idx, val = G.dense_to_csr(np.zeros(shape, np.float32))
        assert counts.tolist() == [0] * shape[0] and idx.size == 0 and val.size == 0
        assert G.check_csr(counts, idx, 0) == 0


def test_csr_rules_of_append():
    ok = (np.array([2, 0, 3], np.uint32), np.array([1, 5, 0, 2, 9], np.uint32))
    assert G.check_csr(*ok) == 0 and G.check_csr(*ok, elements=5) == 0
    assert G.check_csr(*ok, elements=4) == G.INVALID and G.check_csr(*ok, elements=6) == G.INVALID
    assert G.check_csr([2, 0, 3], [1, 1, 0, 2, 9]) == G.INVALID        # an equal neighbour
    assert G.check_csr([2, 0, 3], [1, 5, 0, 9, 2]) == G.INVALID        # descending at a run's last element
    assert G.check_csr([2, 0, 3], [5, 9, 0, 2, 3]) == 0                # a new run may start below the one before
    assert G.check_csr([4096], np.arange(4096)) == 0
    assert G.check_csr([4097], np.arange(4097)) == G.INVALID
    assert G.check_csr([3], [1, 2]) == G.INVALID                       # counts beyond the arrays


def test_the_fp64_scorer_agrees_on_the_converted_rows():
    rng = np.random.default_rng(5)
    n, nq, dim = 40, 7, 90
    rows = np.where(rng.random((n, dim)) < 0.2, rng.uniform(-1, 1, (n, dim)), 0.0).astype(np.float32)
    qs = np.where(rng.random((nq, dim)) < 0.3, rng.uniform(-1, 1, (nq, dim)), 0.0).astype(np.float32)
    rows[3] = 0.0
    qs[2] = 0.0
    rows[5, 7] = -0.0
    ref, A = R.sparse_reference(G.dense_to_csr(rows), G.dense_to_csr(qs))
    dense = -(qs.astype(np.float64) @ rows.astype(np.float64).T)
    # both are fp64 sums of the same exact products in different orders: (terms + 1) * 2^-52 * sum |terms| bounds either
    assert np.all(np.abs(ref - dense) <= (dim + 1) * 2.0 ** -52 * A + 0.0)
    assert np.all(ref[2] == 0.0) and np.all(ref[:, 3] == 0.0)
