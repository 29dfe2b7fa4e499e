"""Reference for feeding the sparse index from device memory (numpy only): dense rows -> CSR, append's validation of CSR, and a
store-equality checker for two handles.

A dense row becomes the pairs (column, value) of its elements that are not zero, in column order.  "Not zero" is the IEEE
comparison on the element as it is: +0.0 and -0.0 are dropped, every other bit pattern is kept and comes out with its bits
unchanged — subnormals, inf and NaN included.  Column order makes every run strictly ascending.
"""
import numpy as np

INVALID = -31                   # ZVEC_HIP_ERR_INVALID_ARGUMENT
MAX_COUNT = 4096                # PARAM_FLAT_SPARSE_MAX_DIM_SIZE
FLT_MAX = float(np.finfo(np.float32).max)


def raw(values):
    """the bits of fp32 / fp16 values"""
    v = np.ascontiguousarray(values)
    return v.view(np.uint16 if v.dtype == np.float16 else np.uint32)


def dense_to_csr(matrix):
    """(counts uint32 [n], indices uint32, values of the matrix's type): `!= 0` per row, column order, values bit for bit"""
    m = np.asarray(matrix)
    assert m.ndim == 2 and m.dtype in (np.float32, np.float16)
    with np.errstate(invalid="ignore"):
        keep = m != 0                                   # (NaN != 0; -0.0 == 0; numpy flushes no subnormal)
    counts = keep.sum(axis=1).astype(np.uint32)
    indices = np.nonzero(keep)[1].astype(np.uint32)     # (row-major: column order inside a row)
    values = m[keep].astype(m.dtype, copy=True)
    return counts, indices, values


def check_csr(counts, indices, elements=None):
    """append's rules for a batch: at most 4096 pairs a run, every run strictly ascending, and (elements given) the counts summing
    to it.  0 or INVALID."""
    counts = np.asarray(counts, np.uint32).astype(np.int64)
    indices = np.asarray(indices, np.uint32).astype(np.int64)
    if (counts > MAX_COUNT).any():
        return INVALID
    total = int(counts.sum())
    if elements is not None and total != int(elements):
        return INVALID
    if total > indices.size:
        return INVALID
    o = 0
    for c in counts:
        run = indices[o:o + c]
        if c > 1 and (run[1:] <= run[:-1]).any():
            return INVALID
        o += int(c)
    return 0


def search_all(se, topk=None):
    """one search that returns every row that is not a hole: an empty query (every row scores 0 under InnerProductSparse and its
    own sum of squares under SquaredEuclideanSparse), topk = the row count.  (keys, scores, counts) as the call left them."""
    n = se.count()
    ctx = se.create_context()
    ctx.set_topk(max(1, n if topk is None else topk))
    assert se.search_impl(np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, se.np_dtype), 1, ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def read_store(se):
    """everything the C ABI tells about a store: per position the row as stored (indices, value bits), the counts, the holes, and
    the keys as one search over every row returns them"""
    rows = []
    for p in range(se.count()):
        i, v = se.get_vector_by_id(p)
        rows.append((i.tobytes(), raw(v).tobytes()))
    keys, scores, counts = search_all(se)
    return {"rows": rows, "count": se.count(), "elements": se.element_count(), "holes": se.holes(),
            "keys": keys.tobytes(), "scores": scores.tobytes(), "found": counts.tobytes()}


def assert_same_store(a, b):
    """a, b: read_store's of two handles (or of one handle at two times)"""
    assert a["count"] == b["count"], (a["count"], b["count"])
    assert a["elements"] == b["elements"], (a["elements"], b["elements"])
    assert a["holes"] == b["holes"], (a["holes"], b["holes"])
    for p, (x, y) in enumerate(zip(a["rows"], b["rows"])):
        assert x[0] == y[0], (p, "indices differ")
        assert x[1] == y[1], (p, "value bits differ")
    assert a["found"] == b["found"] and a["keys"] == b["keys"] and a["scores"] == b["scores"], "the search over every row differs"
