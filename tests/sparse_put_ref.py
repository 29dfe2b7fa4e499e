"""A plain Python model of a sparse index under add-with-id (zvec_hip_sparse_put), and the checker that compares what a handle
reads back with it.  numpy only.

The model follows FlatSparseStreamerEntity::add_vector_with_id (flat_sparse_streamer_entity.cc:708-783) literally, one row after
the other in call order:
    id == count  the row is appended
    id >  count  positions [count, id) are padded with empty rows under the invalid key first (holes), then the row is appended
    id <  count  the row at that position is replaced; a hole that is written stops being a hole
The key of a written row is its id unless the call brings keys of its own.

A read-back is a dict: rows (a list of (indices uint32, values) per position, as stored), keys (uint64 per position), hole (bool per
position: no search returns it), holes (the handle's hole count), count (rows) and elements (stored pairs).  Values are compared as
bits, so -0.0, denormals and halves are held exactly."""
import numpy as np

INVALID_KEY = 0xffffffffffffffff
NP = {"fp32": np.float32, "fp16": np.float16}


def raw(values):
    """the bits of fp32 / fp16 values"""
    v = np.ascontiguousarray(values)
    return v.view(np.uint16 if v.dtype.itemsize == 2 else np.uint32)


class PutModel:
    def __init__(self, dtype):
        self.np_dtype = NP[dtype]
        self.rows = []            # per position: (indices uint32, values np_dtype)
        self.keys = []            # per position: int
        self.holes = set()

    def empty_row(self):
        return np.zeros(0, np.uint32), np.zeros(0, self.np_dtype)

    def count(self):
        return len(self.rows)

    def elements(self):
        return sum(int(r[0].size) for r in self.rows)

    def copy(self):
        m = PutModel("fp16" if self.np_dtype == np.float16 else "fp32")
        m.rows = [(i.copy(), v.copy()) for i, v in self.rows]
        m.keys = list(self.keys)
        m.holes = set(self.holes)
        return m

    def batch(self):
        """the rows as one CSR batch (counts, indices, values), holes as empty rows"""
        counts = np.array([r[0].size for r in self.rows], np.uint32)
        idx = np.concatenate([r[0] for r in self.rows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        val = np.concatenate([r[1] for r in self.rows] + [np.zeros(0, self.np_dtype)]).astype(self.np_dtype)
        return counts, idx, val

    def hole_mask(self):
        m = np.zeros(len(self.rows), bool)
        m[sorted(self.holes)] = True
        return m


def apply_put(model, ids, counts, indices, values, keys=None):
    """add_vector_with_id for every row of the call, in call order"""
    indices = np.asarray(indices, np.uint32)
    values = np.asarray(values, model.np_dtype)
    o = 0
    for i, doc in enumerate(ids):
        doc, c = int(doc), int(counts[i])
        row = (indices[o:o + c].copy(), values[o:o + c].copy())
        o += c
        key = doc if keys is None else int(keys[i])
        n = len(model.rows)
        if doc > n:
            for p in range(n, doc):
                model.rows.append(model.empty_row())
                model.keys.append(INVALID_KEY)
                model.holes.add(p)
        if doc == len(model.rows):
            model.rows.append(row)
            model.keys.append(key)
        else:
            model.rows[doc] = row
            model.keys[doc] = key
            model.holes.discard(doc)
    assert o == indices.size == values.size


def pack(rows, np_dtype):
    """rows [(indices, values)] -> (counts, indices, values) of one call"""
    counts = np.array([len(r[0]) for r in rows], np.uint32)
    idx = np.concatenate([np.asarray(r[0], np.uint32) for r in rows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    val = np.concatenate([np.asarray(r[1], np_dtype) for r in rows] + [np.zeros(0, np_dtype)]).astype(np_dtype)
    return counts, idx, val


def random_row(rng, length, vocab, np_dtype, specials=True):
    """`length` strictly ascending indices below `vocab`, values of mixed sign; specials: with a -0.0 and a denormal among them
    (bit patterns a copy has to keep; not for rows that are scored against a band, whose products must not underflow)"""
    idx = np.sort(rng.choice(vocab, int(length), replace=False)).astype(np.uint32)
    val = rng.uniform(-1.0, 1.0, int(length)).astype(np_dtype)
    if specials and length >= 3:
        val[int(rng.integers(length))] = np_dtype(-0.0)
        val[int(rng.integers(length))] = np.finfo(np_dtype).smallest_subnormal
    return idx, val


def read_back_of_model(model):
    """the read-back a faultless handle gives for `model`"""
    return {"rows": [(i.copy(), v.copy()) for i, v in model.rows], "keys": np.array(model.keys, np.uint64),
            "hole": model.hole_mask(), "holes": len(model.holes), "count": model.count(), "elements": model.elements()}


def check_store(got, model):
    """assert that a read-back equals the model: counts, every row bit for bit, every key, the holes"""
    n = model.count()
    assert got["count"] == n, ("rows", got["count"], n)
    assert got["elements"] == model.elements(), ("elements", got["elements"], model.elements())
    assert got["holes"] == len(model.holes), ("holes", got["holes"], len(model.holes))
    assert len(got["rows"]) == n and len(got["keys"]) == n and len(got["hole"]) == n
    want_hole = model.hole_mask()
    for r in range(n):
        wi, wv = model.rows[r]
        gi, gv = got["rows"][r]
        assert np.asarray(gi).dtype == np.uint32 and np.array_equal(gi, wi), ("indices of row", r)
        assert np.asarray(gv).dtype == model.np_dtype and raw(gv).tobytes() == raw(wv).tobytes(), ("values of row", r)
        assert bool(got["hole"][r]) == bool(want_hole[r]), ("hole", r, bool(got["hole"][r]))
        assert int(got["keys"][r]) == int(model.keys[r]), ("key of row", r, int(got["keys"][r]), int(model.keys[r]))


def read_store(se):
    """the read-back of a zvec_amd.HipFlatSparseStreamer: the rows through get_vector_by_id, and key and hole of every position
    through ONE listed-rows search of an empty query, query r against position r alone (a hole returns nothing; under either
    metric an empty query scores every other row finitely).
    What this cannot see: the key STORED at a hole.  Every entry that returns keys applies the hole bits first, so no call of the
    library reads the key column at a hole; keys[r] of a hole is filled in here as INVALID_KEY, not read from the device, and "hole"
    is what the hole bits say.  The invalid key that the library writes at padded positions is therefore not held by any test; it
    matters only to a reader of the raw column, which the C ABI does not offer."""
    import ctypes as C
    from zvec_amd import _lib

    def ptr(a):
        return C.c_void_p(a.ctypes.data)

    n = se.count()
    rows = [se.get_vector_by_id(r) for r in range(n)]
    keys = np.full(n, INVALID_KEY, np.uint64)
    hole = np.ones(n, bool)
    if n:
        qc, ids, offs = np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32)
        out_k, out_s, out_c = np.zeros((n, 1), np.uint64), np.zeros((n, 1), np.float32), np.zeros(n, np.uint32)
        rc = _lib.lib().zvec_hip_sparse_search_by_ids(se._h, None, ptr(qc), None, None, n, ptr(ids), ptr(offs), 1,
                                                      float(np.finfo(np.float32).max), None, ptr(out_k), ptr(out_s), ptr(out_c))
        assert rc == 0, rc
        hole = out_c == 0
        keys = np.where(hole, np.uint64(INVALID_KEY), out_k[:, 0])
    return {"rows": rows, "keys": keys, "hole": hole, "holes": se.holes(), "count": n, "elements": se.element_count()}
