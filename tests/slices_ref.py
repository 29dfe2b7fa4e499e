"""The fixtures of the query-slicing tests (numpy only; nothing here touches the GPU or the library).

Six host loops cut a batch of queries into slices and address everything of a slice at an offset q0 ("Query slices"):

  loop  where                                             slice width                                        row_floats
  1     flat_scan_prepared, dense-score path (large k)    dense_sub_batch(count, row_floats)                 ceil(n / 128) * 128
  2     flat_scan_hamming, k > 128                        dense_sub_batch(count, row_floats)                 ceil(n / 128) * 128
  3     sparse_search_locked, k > 128, no twin            dense_sub_batch(count, row_floats)                 n
  4     sparse_inverted_search_locked                     dense_sub_batch(count, row_floats)                 ceil(n / 4096) * 4096
  5     zvec_hip_sparse_search_grouped                    dense_sub_batch(min(count, 32768), row_floats)     n
  6     zvec_hip_sparse_search_grouped_by_ids             32768                                              -

dense_sub_batch is restated here; tests/test_slices_reference_cpu.py holds every fixture to "at least two slices" under it, so a
fixture that stops slicing fails on the CPU instead of passing on the GPU.  checked_queries() is built from the restated formula
(not from fixed ranges): query 0, the last query and three queries on each side of every slice boundary.

Data: small integers everywhere, so every score is exact in fp32 (and every sparse value in fp16) and an answer is held bit for
bit; every query of a batch differs from every other, so an answer computed from, or written to, the wrong slice cannot pass.
The three sparse loops over 2^20 + 37 rows share their rows and queries (their slice widths are all 255), hence one reference."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_group_ref as G  # noqa: E402
import sparse_ref as R  # noqa: E402
from hamming_ref import hamming_reference  # noqa: E402

GIB = 2 ** 30
N_BIG = 2 ** 20 + 37
VOCAB = 300
NEAR = 3                     # checked queries on each side of a boundary

# the fused limits the large-k routes lie beyond
HAM_FUSED_MAX_K = 128
SPARSE_FUSED_MAX_K = 128
SPARSE_QB, HAM_QB, WIDE_ROWS = 64, 32, 128       # queries per sparse plan block, per Hamming block, per 8-wave scan tile


def dense_sub_batch(cap, row_floats):
    """api_flat_scan.inc.h: queries per sub-batch of a [query][row_floats] fp32 matrix of at most 1 GiB"""
    return max(1, min(cap, GIB // (row_floats * 4)))


def flat_fused_max_k():
    """the largest k pick_ng(count, k) still finds a fused tile for: scan_lds_bytes(1, k) <= LDS_LIMIT - 1024 with
    scan_lds_bytes(ng, k) = (2 rows TILE_K + 2 SLAB + 7 rows + 4 + 2 rows k) * 4, rows = 32 ng, TILE_K = 32, SLAB = 128 * 32,
    LDS_LIMIT = 160 KiB"""
    rows, tile_k, slab, limit = 32, 32, 128 * 32, 160 * 1024 - 1024
    return (limit // 4 - (2 * rows * tile_k + 2 * slab + 7 * rows + 4)) // (2 * rows)


FIXTURES = {
    "flat_large_k":          dict(loop=1, n=N_BIG, count=300, k=600, dim=8, dtype="fp32", metrics=("SquaredEuclidean", "InnerProduct")),
    "hamming":               dict(loop=2, n=N_BIG, count=300, k=129, dim=64, dtype="binary32", metrics=("Hamming",)),
    "sparse_scan":           dict(loop=3, n=N_BIG, count=300, k=129, dtype="fp32", metrics=("InnerProductSparse",)),
    "sparse_inverted":       dict(loop=4, n=N_BIG, count=300, k=10, dtype="fp32", metrics=("InnerProductSparse",)),
    "sparse_group_gib":      dict(loop=5, n=N_BIG, count=300, gnum=4, gk=3, ngroups=50, dtype="fp32", metrics=("InnerProductSparse",)),
    "sparse_group_32768":    dict(loop=5, n=200, count=32770, gnum=3, gk=2, ngroups=10, dtype="fp32", metrics=("InnerProductSparse",)),
    "sparse_group_ids_32768": dict(loop=6, n=200, count=32770, gnum=3, gk=2, ngroups=10, dtype="fp32", metrics=("InnerProductSparse",)),
}
GIB_FIXTURES = [name for name, fx in FIXTURES.items() if fx["n"] == N_BIG]
SPARSE_FIXTURES = [name for name, fx in FIXTURES.items() if fx["loop"] >= 3]


def row_floats(fx):
    """floats of one query's row of the score matrix (None: loop 6 has no such cap)"""
    n, loop = fx["n"], fx["loop"]
    if loop in (1, 2):
        return (n + 127) // 128 * 128
    if loop in (3, 5):
        return n
    if loop == 4:
        return (n + 4095) // 4096 * 4096
    return None


def slice_width(fx):
    if fx["loop"] == 6:
        return 32768
    cap = min(fx["count"], 32768) if fx["loop"] == 5 else fx["count"]
    return dense_sub_batch(cap, row_floats(fx))


def boundaries(fx):
    """the first query of every slice but the first"""
    return list(range(slice_width(fx), fx["count"], slice_width(fx)))


def slice_of(fx, q):
    return q // slice_width(fx)


def checked_queries(fx):
    """query 0, the last one, and NEAR queries on each side of every boundary — from the restated formula"""
    s = {0, fx["count"] - 1}
    for b in boundaries(fx):
        s.update(range(max(0, b - NEAR), min(fx["count"], b + NEAR)))
    return sorted(s)


def where(fx, q):
    """for assertion messages: the query and the slice it lies in"""
    return "query %d (slice %d of %d, width %d)" % (q, slice_of(fx, q), len(boundaries(fx)) + 1, slice_width(fx))


# ---- data -------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def drop(prefix):
    """forget the cached arrays whose key starts with `prefix` (the large references, once their last user is through)"""
    for key in [k for k in _CACHE if k[0].startswith(prefix)]:
        del _CACHE[key]


def all_differ(rows):
    """no two rows of a 2-D array are equal"""
    return np.unique(np.ascontiguousarray(rows), axis=0).shape[0] == len(rows)


def dense_data(name="flat_large_k"):
    """(rows [n][dim], queries [count][dim]) fp32, integers in [-6, 6].  One pair of queries is planted: query 0 has a tiny norm
    (5) and the first query of the second slice the largest there is (36 per dimension).  A second slice scored with the first
    slice's norms (`qnorm` not offset) then gives that query L2 scores that are too low by 36 dim - 5; the scan clamps a dumped
    L2 score at 0, so most rows tie at 0, the selection falls back on the position and the refined list is not the k nearest
    (norm_mutant_lists, held on the CPU).  With random norms on both sides the shift is small and clamps next to nothing."""
    fx = FIXTURES[name]

    def make():
        rng = np.random.default_rng([101, fx["n"], fx["dim"]])
        base = rng.integers(-6, 7, (fx["n"], fx["dim"])).astype(np.float32)
        q = rng.integers(-6, 7, (fx["count"], fx["dim"])).astype(np.float32)
        sign = np.where(np.arange(fx["dim"]) % 3 == 1, -1.0, 1.0).astype(np.float32)
        q[0] = sign * (np.arange(fx["dim"]) % 8 < 5)              # five entries of +-1, the rest 0
        q[slice_width(fx)] = 6 * sign
        return base, q
    return _once(("dense", name), make)


def norm_mutant_lists(name="flat_large_k"):
    """what the L2 search would return for the checked queries of a later slice if the scan read the FIRST slice's norms
    (`qnorm + q0` -> `qnorm`): the dumped score of query q is max(true - |q|^2 + |q - q0|^2, 0), the k best by (score, position)
    are selected and re-scored directly.  Returns {query: (positions [k], true distances [k], ascending)}."""
    fx = FIXTURES[name]
    _, q = dense_data(name)
    ref = dense_reference("SquaredEuclidean", name)
    qn = (q.astype(np.float64) ** 2).sum(1)
    w = slice_width(fx)
    out = {}
    for j, qi in enumerate(checked_queries(fx)):
        if qi >= w:
            dumped = np.maximum(ref[j] - qn[qi] + qn[qi - qi // w * w], 0.0)
            pos = np.argsort(dumped, kind="stable")[:fx["k"]]
            pos = pos[np.argsort(ref[j][pos], kind="stable")]
            out[qi] = (pos, ref[j][pos])
    return out


def hamming_data(name="hamming"):
    """(rows, queries) uint32 words of random bits"""
    fx = FIXTURES[name]

    def make():
        rng = np.random.default_rng([103, fx["n"], fx["dim"]])
        words = fx["dim"] // 32
        return (rng.integers(0, 2 ** 32, (fx["n"], words), dtype=np.uint64).astype(np.uint32),
                rng.integers(0, 2 ** 32, (fx["count"], words), dtype=np.uint64).astype(np.uint32))
    return _once(("hamming", name), make)


def _int_values(rng, size):
    return (rng.integers(1, 7, size) * rng.choice([-1, 1], size)).astype(np.float32)


def sparse_rows(n):
    """(counts, indices, values): four draws from the vocabulary per row, duplicates dropped (1 .. 4 elements, mostly 4), ascending;
    non-zero integer values |v| <= 6"""
    def make():
        rng = np.random.default_rng([107, n])
        idx = np.sort(rng.integers(0, VOCAB, (n, 4)), axis=1)
        keep = np.ones((n, 4), bool)
        keep[:, 1:] = idx[:, 1:] != idx[:, :-1]
        indices = idx[keep].astype(np.uint32)
        return keep.sum(1).astype(np.uint32), indices, _int_values(rng, indices.size)
    return _once(("sparse_rows", n), make)


def sparse_queries(count):
    """(counts, indices, values): 3 .. 8 distinct terms per query, the lengths varying from query to query (so the queries' offsets
    into the index and value arrays are no multiple of anything), non-zero integer values |v| <= 6"""
    def make():
        rng = np.random.default_rng([109, count])
        lengths = rng.integers(3, 9, count)
        pick = np.argpartition(rng.random((count, VOCAB)), 8, axis=1)[:, :8]          # 8 distinct terms per query
        pick = np.where(np.arange(8)[None, :] < lengths[:, None], pick, VOCAB)          # the first `length` of them
        pick = np.sort(pick, axis=1)
        indices = pick[pick < VOCAB].astype(np.uint32)
        return lengths.astype(np.uint32), indices, _int_values(rng, indices.size)
    return _once(("sparse_queries", count), make)


def sparse_queries_differ(queries):
    c, i, v = queries
    o = R.offsets(c)
    return len({(i[o[q]:o[q + 1]].tobytes(), v[o[q]:o[q + 1]].tobytes()) for q in range(len(c))}) == len(c)


def sparse_key_of(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)


def group_of(name):
    fx = FIXTURES[name]
    return _once(("group_of", name), lambda: np.random.default_rng([113, fx["n"]]).integers(0, fx["ngroups"], fx["n"]).astype(np.uint32))


def id_lists(name="sparse_group_ids_32768"):
    """per query 1 .. 4 positions (a position may come twice)"""
    fx = FIXTURES[name]

    def make():
        rng = np.random.default_rng([127, fx["count"]])
        return tuple(rng.integers(0, fx["n"], int(m)).astype(np.uint32) for m in rng.integers(1, 5, fx["count"]))
    return _once(("id_lists", name), make)


def exclude_mask(n):
    """bool [n]: a seeded 45 % of the rows.  Just under half on purpose: with half or more of the rows excluded a flat search
    compacts the kept rows first (flat_scan_prepared, "Sparse keep-set"), the score matrix of the compacted copy is half as wide
    and the batch is no longer sliced."""
    return _once(("exclude", n), lambda: np.random.default_rng([131, n]).random(n) < 0.45)


def words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


# ---- references, for the checked queries only ------------------------------------------------------------------------------------------
def top_lists(scores, k, admissible=None):
    """(positions [nq][k], scores [nq][k] fp32, counts [nq]) of an [nq][n] score matrix: the k best by (score, position)"""
    nq, n = scores.shape
    pos = np.zeros((nq, k), np.uint64)
    out = np.zeros((nq, k), np.float32)
    cnt = np.zeros(nq, np.uint32)
    for q in range(nq):
        cand = np.arange(n) if admissible is None else np.nonzero(admissible)[0]
        order = cand[np.argsort(scores[q, cand], kind="stable")][:k]
        cnt[q] = order.size
        pos[q, :order.size] = order
        out[q, :order.size] = scores[q, order]
    return pos, out, cnt


def check_exact_list(keys, scores, count, ref_row, k, key_of, admissible=None, what=""):
    """one query's list (keys [k], scores [k], count) against its exact reference scores ref_row [n] (every score a number fp32
    holds): the scores are, rank by rank, the k best of the admissible rows; every key is a stored one, admissible, listed once,
    and its row scores exactly what the list says.  Free: which rows of the k-th score are listed and the order of equal scores."""
    n = ref_row.size
    adm = np.ones(n, bool) if admissible is None else np.asarray(admissible, bool)
    want = np.sort(ref_row[adm])[:k]
    c = int(count)
    assert c == want.size, "%s: %d entries, reference %d" % (what, c, want.size)
    got_s = np.asarray(scores[:c], np.float64)
    assert np.array_equal(got_s, want), "%s: scores differ at ranks %r\n got %r\nwant %r" % (
        what, np.nonzero(got_s != want)[0][:8], got_s[:8], want[:8])
    got_k = np.asarray(keys[:c], np.uint64)
    order = np.argsort(key_of, kind="stable")
    at = np.minimum(np.searchsorted(key_of, got_k, sorter=order), n - 1)
    pos = order[at]
    assert np.array_equal(np.asarray(key_of, np.uint64)[pos], got_k), "%s: unknown keys %r" % (what, got_k[np.asarray(key_of)[pos] != got_k][:8])
    assert np.unique(pos).size == c, "%s: a row is listed twice" % what
    assert np.all(adm[pos]), "%s: excluded rows listed: %r" % (what, pos[~adm[pos]][:8])
    own = ref_row[pos]
    assert np.array_equal(own, got_s), "%s: rows %r are listed with scores %r, their own scores are %r" % (
        what, pos[own != got_s][:8], got_s[own != got_s][:8], own[own != got_s][:8])


def dense_reference(metric, name="flat_large_k"):
    """fp64 scores [checked][n] of the checked queries: the squared distance summed directly, or minus the dot product"""
    def make():
        base, q = dense_data(name)
        sel = checked_queries(FIXTURES[name])
        b64 = base.astype(np.float64)
        out = np.empty((len(sel), len(base)))
        for j, qi in enumerate(sel):
            q64 = q[qi].astype(np.float64)
            out[j] = ((b64 - q64[None, :]) ** 2).sum(1) if metric == "SquaredEuclidean" else -(b64 @ q64)
        return out
    return _once(("ref_dense", name, metric), make)


def hamming_scores(name="hamming"):
    def make():
        base, q = hamming_data(name)
        return hamming_reference(base, q[checked_queries(FIXTURES[name])], chunk=1 << 16)
    return _once(("ref_hamming", name), make)


def sparse_case(name):
    """(rows, the checked queries as a batch, ref, A, m) in the layout of sparse_ref.make_case"""
    fx = FIXTURES[name]
    sel = checked_queries(fx)

    def make():
        rows = sparse_rows(fx["n"])
        qs = G.take_queries(sparse_queries(fx["count"]), sel)
        ref, A = R.sparse_reference(rows, qs)
        return rows, qs, ref, A, R.shared_counts(rows, qs)
    # (the fixtures over the same rows, queries and checked set share one reference)
    return _once(("ref_sparse", fx["n"], fx["count"], tuple(sel)), make)


def group_want(name):
    """the rendered group-by answer of the checked queries (sparse_group_ref.render)"""
    fx = FIXTURES[name]
    sel = checked_queries(fx)

    def make():
        lists = [id_lists(name)[q] for q in sel] if fx["loop"] == 6 else None
        r = G.group_reference(sparse_case(name), group_of(name), fx["ngroups"], fx["gnum"], fx["gk"], candidates=lists)
        return G.render(r["queries"], fx["gnum"], fx["gk"], sparse_key_of(fx["n"]))
    return _once(("ref_group", name), make)
