"""Fixtures of the fp16 HNSW handle (zvec_hip_hnsw_create_typed(ZVEC_HIP_DT_FP16), DESIGN §3c "fp16 rows").

A twin case is (fp16 rows, fp16 queries, a graph or build parameters).  The contract: an fp16 handle answers bit for bit as W, the fp32
handle given widen(rows) and widen(queries).  Two kinds of data:
  exact   the integer rows of hnsw_ref.exact_rows ([-8, 8], dim <= 128): exact in binary16, every distance an exact fp32 integer in
          any summation order, so the fp64 models of hnsw_ref / hnsw_build_ref / hnsw_add_ref apply as they stand;
  real    standard_normal rounded to binary16, with half subnormals (k * 2^-24), -0.0 and the largest finite half planted: no model,
          the comparison is with W alone.
tests/test_hnsw_f16_reference_cpu.py asserts what the fixtures must show."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402

HALF_MAX = 65504.0                  # the largest finite binary16
SUB = 2.0 ** -24                    # the smallest positive binary16 (subnormal); the subnormals are k * SUB, k < 1024

Twin = collections.namedtuple("Twin", "rows16 queries16 graph")      # graph: hnsw_ref.Graph over widen(rows16)


def widen(a):
    """binary16 -> fp32, exact"""
    a = np.asarray(a)
    assert a.dtype == np.float16
    return a.astype(np.float32)


def is_half(a):
    """every value of the fp32 array survives fp32 -> binary16 -> fp32"""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float16).astype(np.float32).view(np.uint32), a.view(np.uint32)))


# ---- exact ---------------------------------------------------------------------------------------------------------------------
EXACT_DIMS = (1, 3, 4, 5, 63, 64, 65, 128)      # padding; one 4-element step; exactly one 16-lane step (64) and one element into the second
EXACT_N, EXACT_M, EXACT_Q = 300, 6, 12


@functools.lru_cache(maxsize=None)
def exact_twin(dim):
    g = H.exact_graph(EXACT_N, dim, EXACT_M)
    q = H.exact_queries(g, np.random.default_rng([16, dim]), EXACT_Q)
    return Twin(g.rows.astype(np.float16), q.astype(np.float16), g)


def usable_hand_made():
    """the hand-made graphs of hnsw_ref whose rows are binary16 values"""
    return collections.OrderedDict((k, f) for k, f in H.HAND_MADE.items() if is_half(f().rows))


HAND_QUERIES = np.array([[0, 0, 0, 0], [10, 0, 0, 0], [30, 0, 0, 0], [12, 0, 0, 0], [8, 0, 0, 0]], np.float16)


def build_rows(n, dim):
    """(fp16 rows, Params, levels) of the build and add cases on exact data"""
    return B.base_rows(n, dim).astype(np.float16), B.params(m=4, m0=8, ef_construction=16), B.mid_levels(n, 4)


# ---- real ----------------------------------------------------------------------------------------------------------------------
REAL_DIMS = (7, 64, 68, 260, 772)   # 772 halves: a 1544-byte row, off the 16-byte grid; 260: past the unroll-by-4 tail of the row loop
REAL_N, REAL_Q, REAL_M = 2000, 24, 8
SPILL_N, SPILL_EXCLUDED, SPILL_DIM, SPILL_M = 1500, 1400, 260, 32     # (lists of 64: the candidate set outgrows the pops, see spill_twin)
BUILD_N, BUILD_ADDS = 600, (1, 64, 300)
BUILD_PARAMS = B.params(m=8, m0=16, ef_construction=32)
PLANT_DIM = 68
PLANT_ROW, PLANT_MAX_ROW = 17, 23   # a row of subnormals, zeros and -0.0 only; the row whose coordinate 5 is the largest finite half
PLANT_QUERY = 3                     # a query of subnormals and -0.0 only


def real_rows(n, dim, seed):
    """standard_normal rounded to binary16 (round to nearest even)"""
    return np.random.default_rng([seed, n, dim]).standard_normal((n, dim)).astype(np.float16)


def _graph(rows16, m, seed, metric="l2"):
    return H.build_graph(widen(rows16), m, 24, seed, metric)


@functools.lru_cache(maxsize=None)
def real_twin(dim, n=REAL_N):
    rows = real_rows(n, dim, 1)
    return Twin(rows, real_rows(REAL_Q, dim, 2), _graph(rows, REAL_M, dim))


@functools.lru_cache(maxsize=None)
def spill_twin():
    """1500 rows of which the last 1400 are excluded (spill_exclude): at ef 512 the result list cannot fill, so every node the walk has
    seen and not yet expanded stays a candidate, and lists of 64 bring them in faster than the walk expands them — more than the 1024
    candidates the kernel holds in LDS are alive at once, and the set moves into the workspace"""
    rows = real_rows(SPILL_N, SPILL_DIM, 1)
    return Twin(rows, real_rows(REAL_Q, SPILL_DIM, 2), _graph(rows, SPILL_M, SPILL_DIM))


def spill_exclude():
    return np.arange(SPILL_N) >= SPILL_N - SPILL_EXCLUDED


def plant(rows, queries):
    """in place: a few dozen half subnormals and -0.0 across the rows, a row and a query made of them alone, and the largest finite
    half in one coordinate of one row"""
    rng = np.random.default_rng(99)
    n, dim = rows.shape
    for k in range(40):
        rows[rng.integers(0, n), rng.integers(0, dim)] = np.float16((1 + rng.integers(0, 1023)) * SUB * (-1) ** k)
    for k in range(10):
        rows[rng.integers(0, n), rng.integers(0, dim)] = np.float16(-0.0)
    sub = (rng.integers(0, 1024, dim) * SUB).astype(np.float16)         # (k = 0 gives +0)
    sub[::7] = np.float16(-0.0)
    rows[PLANT_ROW] = sub
    q = (rng.integers(1, 1024, dim) * SUB * rng.choice([-1.0, 1.0], dim)).astype(np.float16)
    q[::5] = np.float16(-0.0)
    queries[PLANT_QUERY] = q
    queries[PLANT_QUERY + 1, :4] = [np.float16(SUB), np.float16(-SUB), np.float16(-0.0), np.float16(1023 * SUB)]
    rows[PLANT_MAX_ROW, 5] = np.float16(HALF_MAX)
    return rows, queries


@functools.lru_cache(maxsize=None)
def planted_twin():
    rows, q = plant(real_rows(REAL_N, PLANT_DIM, 3), real_rows(REAL_Q, PLANT_DIM, 4))
    return Twin(rows, q, _graph(rows, REAL_M, 5))


def real_levels(n, seed=6):
    return B.levels_model(n, BUILD_PARAMS.scaling_factor, seed)
