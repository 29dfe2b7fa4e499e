"""Python plumbing over the C ABI (include/zvec_hip.h), shaped like the reference's index operators.

The C++ host mirror of the reference interface lives in zvec_amd/csrc/host/ (hip_index.h); this module
is the same surface for Python callers (pytest, bench.py): `search_impl(query, count, ctx)` fills
`ctx.result(i)` with IndexDocument(key, score) lists exactly like
IndexSearcher::search_impl(query, qmeta, count, context) (src/include/zvec/core/framework/
index_runner.h:490-500) and returns 0 or a negative IndexError value (index_error.cc:20-71).
No exceptions cross `search_impl` for argument errors — same contract as the reference — but a
missing HIP library / device raises at construction: there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib

from ._lib import METRIC_L2, METRIC_IP, METRIC_COSINE, METRIC_HAMMING        # noqa: E402
from ._lib import DT_FP32, DT_FP16, DT_BINARY32, DT_BINARY64                 # noqa: E402

_DTYPE_NAMES = {"fp32": DT_FP32, "float32": DT_FP32, "fp16": DT_FP16, "float16": DT_FP16,   # (fp16: what HalfFloatConverter writes)
                "binary32": DT_BINARY32,      # IndexMeta::DT_BINARY32: dim bits as dim // 32 uint32 words
                "binary64": DT_BINARY64}      # IndexMeta::DT_BINARY64: dim bits as dim // 64 uint64 words
_NP_OF = {DT_FP32: np.float32, DT_FP16: np.float16, DT_BINARY32: np.uint32, DT_BINARY64: np.uint64}


def _dtype_of(dtype):
    """IndexMeta::DataType of the rows -> (ABI value, numpy type of a row word): a name, a numpy type or the ABI value.
    Anything else raises."""
    if isinstance(dtype, str):
        if dtype in _DTYPE_NAMES:
            return _DTYPE_NAMES[dtype], _NP_OF[_DTYPE_NAMES[dtype]]
    elif isinstance(dtype, (int, np.integer)) and not isinstance(dtype, bool):
        if int(dtype) in _NP_OF:
            return int(dtype), _NP_OF[int(dtype)]
    else:
        try:
            t = np.dtype(dtype).type
        except TypeError:
            t = None
        for k, v in _NP_OF.items():
            if t is v:
                return k, v
    raise ValueError("zvec_amd: unknown row data type %r" % (dtype,))


def _row_words(dim, dt):
    """row length in words of its numpy type: elements for fp rows, dim // 32 resp. dim // 64 words for bit rows"""
    return int(dim) // 32 if dt == DT_BINARY32 else int(dim) // 64 if dt == DT_BINARY64 else int(dim)


FLT_MAX = float(np.finfo(np.float32).max)

_METRIC_NAMES = {
    "SquaredEuclidean": METRIC_L2,   # src/core/metric/euclidean_metric.cc:743
    "InnerProduct": METRIC_IP,       # src/core/metric/inner_product_metric.cc:256
    "Cosine": METRIC_COSINE,         # src/core/metric/cosine_metric.cc:141
    "Hamming": METRIC_HAMMING,       # src/core/metric/hamming_metric.cc:236 (binary rows only)
}


def metric_from_name(name):
    return _METRIC_NAMES[name]


# the metrics of a sparse index (HipFlatSparseStreamer)
_SPARSE_METRIC_NAMES = {
    "InnerProductSparse": METRIC_IP,         # src/core/metric/inner_product_metric.cc:329
    "SquaredEuclideanSparse": METRIC_L2,     # src/core/metric/euclidean_metric.cc:1027-1095
}


class IndexError_:
    """Negative IndexError values used on this path (index_error.cc:20-71)."""
    Success = 0
    Runtime = -1
    Unsupported = -12
    OutOfRange = -17
    NoMemory = -19
    NoReady = -21
    NoExist = -22
    Mismatch = -24
    InvalidArgument = -31
    NoIndexLoaded = -204
    NoTrained = -205


class IndexDocument:
    """key + score (+ the stored vector when the context asked for it) — index_document.h:207-216 subset"""

    def __init__(self, key, score, vector=None):
        self._key = int(key)
        self._score = float(score)
        self._vector = vector

    def key(self):
        return self._key

    def score(self):
        return self._score

    def vector(self):
        """the stored row (fetch_vector contexts only, index.cc:635-647), else None"""
        return self._vector

    def __repr__(self):
        return "IndexDocument(key=%d, score=%r)" % (self._key, self._score)


class GroupIndexDocument:
    """group id + its documents (GroupIndexDocument, index_document.h:270-314)"""

    def __init__(self, group_id, docs):
        self._group_id, self._docs = group_id, docs

    def group_id(self):
        return self._group_id

    def docs(self):
        return self._docs


class DocFilter:
    """The reference's composite document filter (DocFilter::is_filtered, doc_filter.cc:74-87) as data:
        excluded(id) = deleted.contains(id) || !invert.contains(uint32(id)) || !forward[id]
    delete: bytes of a roaring bitmap — `kind` "roaring32" (roaring_bitmap_portable_serialize), "roaring64map"
    (Roaring64Map::write) or "file" (a delete-store file image incl. its 64-byte header); invert: bytes of a 32-bit
    portable roaring bitmap (ids that MATCH the inverted-index condition); forward: numpy bool array indexed by id
    (or packed LSB-first uint8 bits with `forward_len`).  Every term is optional."""

    KINDS = {"roaring32": _lib.ROARING_32, "roaring64map": _lib.ROARING_64MAP, "file": _lib.ROARING_FILE}

    def __init__(self, delete=None, kind="roaring32", invert=None, forward=None, forward_len=None):
        self.delete = None if delete is None else bytes(delete)
        self.kind = self.KINDS[kind]
        self.invert = None if invert is None else bytes(invert)
        if forward is None:
            self.forward, self.forward_len = None, 0
        elif forward_len is None:
            f = np.ascontiguousarray(forward, bool)
            self.forward, self.forward_len = np.packbits(f, bitorder="little"), int(f.size)
        else:
            self.forward, self.forward_len = np.ascontiguousarray(forward, np.uint8), int(forward_len)

    def _desc(self):
        d = _lib.DocFilterDesc()
        self._keep = []                      # buffers the descriptor points into
        if self.delete is not None:
            buf = C.create_string_buffer(self.delete, len(self.delete))
            self._keep.append(buf)
            d.delete_bitmap, d.delete_bytes, d.delete_kind = C.addressof(buf), len(self.delete), self.kind
        if self.invert is not None:
            buf = C.create_string_buffer(self.invert, len(self.invert))
            self._keep.append(buf)
            d.invert_bitmap, d.invert_bytes = C.addressof(buf), len(self.invert)
        if self.forward is not None:
            d.forward_bits, d.forward_len = self.forward.ctypes.data, self.forward_len
        return d


class IndexContext:
    """IndexContext subset used by the scan path (index_context.h:123-195): topk, filter, threshold,
    per-query result lists.  Owns one HIP stream + workspace (zvec_hip_ctx_t)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_ctx_create(device, C.byref(self._h)), "zvec_hip_ctx_create")
        self._topk = 0
        self._threshold = FLT_MAX
        self._exclude = None      # numpy uint64 words (host) — materialised IndexFilter
        self._filter_fn = None
        self._doc_filter = None   # DocFilter: materialised by zvec_hip_*_build_filter
        self._fetch_vector = False
        self._scan_ratio, self._bf_threshold = None, None   # update(params) overrides of the IVF searcher's defaults
        self._group_num, self._group_topk, self._group_by = 0, 0, None
        self._group_results = []
        self._group_cache = None  # (fn, n) -> (group number of every position, group ids)
        self._results = []
        self.keys = None
        self.scores = None
        self.counts = None

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_ctx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- reference surface -------------------------------------------------------------------------
    def set_topk(self, topk):
        self._topk = int(topk)

    def topk(self):
        return self._topk

    def set_fetch_vector(self, enable):
        """IndexContext::set_fetch_vector (index_context.h:139): result documents carry their stored vectors."""
        self._fetch_vector = bool(enable)

    def fetch_vector(self):
        return self._fetch_vector

    def set_group_params(self, group_num, group_topk):
        """IndexContext::set_group_params (index_context.h:129; flat_streamer_context.h:187-191): group_num > 0 turns the
        next searches into group-by searches"""
        self._group_num, self._group_topk = int(group_num), int(group_topk)

    def set_group_by(self, fn):
        """IndexGroupBy: callable(key) -> group id (a string in the reference; any hashable here)"""
        self._group_by = fn
        self._group_cache = None

    def reset_group_by(self):
        self._group_by = None
        self._group_cache = None

    def group_by_search(self):
        return self._group_num > 0

    def group_result(self, index=0):
        """IndexGroupDocumentList of query `index`: groups best first, documents ascending by score"""
        return self._group_results[index]

    def _groups_for(self, keys_of_positions):
        """the group_by callback swept once over the stored keys (cached while the key list and the callback are the
        same): dense group numbers per position + the ids they stand for"""
        n = len(keys_of_positions)
        if self._group_cache is not None and self._group_cache[0] is self._group_by and self._group_cache[1] == n:
            return self._group_cache[2], self._group_cache[3]
        ids, number_of = [], {}
        of = np.empty(n, np.uint32)
        for i, k in enumerate(keys_of_positions):
            g = self._group_by(int(k))
            j = number_of.get(g)
            if j is None:
                j = number_of[g] = len(ids)
                ids.append(g)
            of[i] = j
        self._group_cache = (self._group_by, n, of, ids)
        return of, ids

    def _set_group_results(self, ids, groups, ngroups, keys, scores, counts, vectors_of=None):
        self.group_keys, self.group_scores, self.group_counts, self.group_numbers, self.group_ngroups = keys, scores, counts, groups, ngroups
        self._group_results = []
        for q in range(keys.shape[0]):
            lst = []
            for s in range(int(ngroups[q])):
                c = int(counts[q, s])
                vecs = vectors_of(keys[q, s, :c]) if (self._fetch_vector and vectors_of is not None and c) else None
                lst.append(GroupIndexDocument(ids[int(groups[q, s])],
                                              [IndexDocument(keys[q, s, j], scores[q, s, j], None if vecs is None else vecs[j]) for j in range(c)]))
            self._group_results.append(lst)

    def update(self, params):
        """IndexContext::update(params) (index_context.h:163-166): per-context overrides of the IVF search parameters,
        as IVFSearcherContext::update reads them (ivf_searcher_context.h:61-79) — "proxima.ivf.searcher.scan_ratio" and
        "proxima.ivf.searcher.brute_force_threshold"; a scan_ratio <= 0 is InvalidArgument; flat contexts ignore it."""
        ratio = params.get("proxima.ivf.searcher.scan_ratio", self._scan_ratio)
        if ratio is not None and float(ratio) <= 0.0:
            return IndexError_.InvalidArgument
        self._scan_ratio = None if ratio is None else float(ratio)
        bft = params.get("proxima.ivf.searcher.brute_force_threshold", self._bf_threshold)
        self._bf_threshold = None if bft is None else int(bft)
        return 0

    def set_threshold(self, val):
        self._threshold = float(val)

    def threshold(self):
        return self._threshold

    def set_filter(self, fn):
        """IndexFilter: callable(key) -> True means EXCLUDE (index_filter.h:48-50).  It is swept once
        over the index keys on the host into a bitset at the next search."""
        self._filter_fn = fn
        self._exclude = None

    def set_doc_filter(self, doc_filter):
        """the composite filter as data (DocFilter): materialised on the GPU at the next search, no host sweep."""
        self._doc_filter = doc_filter
        self._filter_fn = None
        self._exclude = None

    def set_exclude_bitset(self, words):
        """side channel: an already materialised predicate, 1 bit per storage position."""
        self._exclude = None if words is None else np.ascontiguousarray(words, np.uint64)
        self._filter_fn = None

    def reset_filter(self):
        self._filter_fn = None
        self._exclude = None
        self._doc_filter = None

    def result(self, index=0):
        return self._results[index]

    def results(self):
        return self._results

    # -- plumbing ----------------------------------------------------------------------------------
    def _exclude_for(self, keys_of_positions):
        if self._exclude is not None:
            return self._exclude
        if self._filter_fn is None:
            return None
        n = len(keys_of_positions)
        mask = np.fromiter((bool(self._filter_fn(int(k))) if k != 0xffffffffffffffff else False for k in keys_of_positions), bool, n)
        words = np.zeros((n + 63) // 64, np.uint64)
        idx = np.nonzero(mask)[0]
        np.bitwise_or.at(words, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
        return words

    def _set_results(self, keys, scores, counts, vectors_of=None):
        """vectors_of: callable(keys 1-D uint64) -> rows, used when fetch_vector is on"""
        self.keys, self.scores, self.counts = keys, scores, counts
        vecs = None
        if self._fetch_vector and vectors_of is not None:
            flat = np.concatenate([keys[q, :int(counts[q])] for q in range(keys.shape[0])]) if keys.shape[0] else np.zeros(0, np.uint64)
            vecs = vectors_of(flat)
        self._results = []
        o = 0
        for q in range(keys.shape[0]):
            c = int(counts[q])
            self._results.append([IndexDocument(keys[q, j], scores[q, j], None if vecs is None else vecs[o + j]) for j in range(c)])
            o += c

    def reform_queries_dev(self, d_in, count, dim, d_out, cosine=False, out_dtype="fp32", stream=None):
        """CosineReformer / HalfFloatReformer on raw fp32 queries already in HBM (device pointers)."""
        dt, _ = _dtype_of(out_dtype)
        _lib.check(_lib.lib().zvec_hip_reform_queries_dev(self._h, C.c_void_p(d_in), int(count), int(dim), int(bool(cosine)), dt,
                                                          C.c_void_p(d_out), C.c_void_p(stream or 0)), "zvec_hip_reform_queries_dev")

    def binary_encode_dev(self, d_in, count, dim, d_out, threshold=0.0, encode_dims=None, stream=None):
        """BinaryConverter / BinaryReformer on fp32 rows already in HBM (device pointers): [count][dim] fp32 -> [count][ceil(dim / 32)]
        uint32 words, bit i of a row = in[i] >= threshold for i < encode_dims (default: dim), every other bit 0.  Only enqueues."""
        _lib.check(_lib.lib().zvec_hip_binary_encode_dev(self._h, C.c_void_p(d_in), int(count), int(dim),
                                                         int(dim if encode_dims is None else encode_dims), float(threshold),
                                                         C.c_void_p(d_out), C.c_void_p(stream or 0)), "zvec_hip_binary_encode_dev")

    def binary_encode(self, rows, threshold=0.0, encode_dims=None):
        """the same for host rows ([count][dim], anything numpy turns into fp32): returns the words, uint32 [count][ceil(dim / 32)]"""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            raise ValueError("zvec_amd: binary_encode takes [count][dim] rows")
        count, dim = rows.shape
        out = np.zeros((count, (dim + 31) // 32), np.uint32)
        _lib.check(_lib.lib().zvec_hip_binary_encode(self._h, _np_ptr(rows), count, dim, int(dim if encode_dims is None else encode_dims),
                                                     float(threshold), _np_ptr(out)), "zvec_hip_binary_encode")
        return out

    def synchronize(self):
        _lib.check(_lib.lib().zvec_hip_ctx_synchronize(self._h), "zvec_hip_ctx_synchronize")

    def set_stream(self, stream_ptr):
        _lib.check(_lib.lib().zvec_hip_ctx_set_stream(self._h, C.c_void_p(stream_ptr)), "ctx_set_stream")

    def set_gate(self, gate):
        """share a Gate with other contexts: their dominant scan kernels then run one after the other while the rest of
        their searches overlaps (zvec_hip_ctx_set_gate); None detaches"""
        _lib.check(_lib.lib().zvec_hip_ctx_set_gate(self._h, gate._h if gate is not None else None), "zvec_hip_ctx_set_gate")
        self._gate = gate        # keeps the gate alive as long as the context uses it

    def profile(self, enable=True):
        _lib.check(_lib.lib().zvec_hip_ctx_profile(self._h, int(enable)), "zvec_hip_ctx_profile")

    def profile_read(self, reset=True):
        n = C.c_uint64(0)
        ms, b, f = C.c_double(0), C.c_double(0), C.c_double(0)
        _lib.check(_lib.lib().zvec_hip_ctx_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(b),
                                                        C.byref(f), int(reset)), "profile_read")
        return {"launches": int(n.value), "scan_ms": ms.value, "bytes": b.value, "flops": f.value}

    def last_route(self):
        """route word of the last flat search on this context (zvec_hip_ctx_last_route: main shape, exclusion, seeding, prefix shape)"""
        r = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_ctx_last_route(self._h, C.byref(r)), "zvec_hip_ctx_last_route")
        return int(r.value)

    def last_ivf_plan(self):
        """route and plan of the last IVF search on this context (zvec_hip_ctx_last_ivf_plan): a dict of the scalars — `route` is one of
        _lib.IVF_ROUTE_* — and, after a tile-route search only, of the plan arrays (uint32); a test and debugging hook"""
        info = _lib.IvfPlanInfo()
        fn = _lib.lib().zvec_hip_ctx_last_ivf_plan
        rc = fn(self._h, C.byref(info), *([None] * 10))
        out = {name: int(getattr(info, name)) for name, _ in _lib.IvfPlanInfo._fields_}
        if rc == _lib.ERR_NO_READY:
            return out
        _lib.check(rc, "zvec_hip_ctx_last_ivf_plan")
        nq, nlist, ncsr = out["nq"], out["nlist"], min(out["csr_len"], out["nq"] * out["nprobe"])
        sizes = (("q_nprobe", nq), ("q_scanned", nq), ("q_nslots", nq), ("slot_begin", nq + 1), ("list_count", nlist),
                 ("list_qoff", nlist + 1), ("item_off", nlist + 1), ("list_tpc", nlist), ("csr_q", ncsr), ("csr_slot", ncsr))
        arrays = [np.zeros(max(n, 1), np.uint32) for _, n in sizes]
        _lib.check(fn(self._h, C.byref(info), *[_np_ptr(a) for a in arrays]), "zvec_hip_ctx_last_ivf_plan")
        out.update({name: a[:n] for (name, n), a in zip(sizes, arrays)})
        return out


def _np_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _FlatBase:
    """Common body of HipFlatStreamer / HipFlatSearcher: one HBM-resident blocked store."""

    def __init__(self, dim, metric=METRIC_L2, device=0, dtype="fp32"):
        if isinstance(metric, str):
            metric = metric_from_name(metric)
        self.dim = int(dim)
        self.metric = metric
        self.device = device
        self.dtype, self.np_dtype = _dtype_of(dtype)
        self.row_words = _row_words(self.dim, self.dtype)     # words of np_dtype per row (== dim for fp rows)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_flat_create(self.dim, self.dtype, metric, device, C.byref(self._h)),
                   "zvec_hip_flat_create")
        self._keys_host = []      # for IndexFilter sweeps

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_flat_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def create_context(self):
        return IndexContext(self.device)

    def count(self):
        n = C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_flat_count(self._h, C.byref(n)), "zvec_hip_flat_count")
        return int(n.value)

    def reserve(self, n):
        return _lib.lib().zvec_hip_flat_reserve(self._h, int(n))

    def add_batch(self, vecs, keys=None):
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        if vecs.ndim != 2 or vecs.shape[1] != self.row_words:
            return IndexError_.InvalidArgument
        n0 = self.count()
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_flat_append(self._h, _np_ptr(vecs), vecs.shape[0], _np_ptr(k))
        if rc == 0:
            self._keys_host.append(np.arange(n0, n0 + vecs.shape[0], dtype=np.uint64) if k is None else k.copy())
        return rc

    def add_batch_dev(self, d_ptr, n, d_keys_ptr=None, stream=None):
        """append rows already resident in HBM (device pointer, [n][dim] fp32 row-major)."""
        n0 = self.count()
        rc = _lib.lib().zvec_hip_flat_append_dev(self._h, C.c_void_p(d_ptr), int(n),
                                                 C.c_void_p(d_keys_ptr) if d_keys_ptr else None,
                                                 C.c_void_p(stream) if stream else None)
        if rc == 0 and d_keys_ptr is None:
            self._keys_host.append(("range", n0, n0 + int(n)))
        return rc

    def add_batch_fp32(self, rows, keys=None, threshold=0.0, encode_dims=None):
        """fp32 rows into a "Hamming" index of binary32 rows (BinaryConverter in front of the builder): [n][dim] rows are turned into
        sign bits on the GPU — bit i = rows[:, i] >= threshold for i < encode_dims (default: all dim values; the reference's converter
        stops at 32 * ceil(dim / 32) // 2, include/zvec_hip.h) — and stored as add_batch stores the same words.  The index must hold
        32 * ceil(dim / 32) bits."""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            return IndexError_.InvalidArgument
        n0 = self.count()
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_flat_append_fp32(self._h, _np_ptr(rows), rows.shape[0], rows.shape[1],
                                                  int(rows.shape[1] if encode_dims is None else encode_dims), float(threshold), _np_ptr(k))
        if rc == 0 and rows.shape[0]:
            self._keys_host.append(np.arange(n0, n0 + rows.shape[0], dtype=np.uint64) if k is None else k.copy())
        return rc

    def add_batch_fp32_dev(self, d_ptr, n, dim, d_keys_ptr=None, threshold=0.0, encode_dims=None, stream=None):
        """add_batch_fp32 for rows already resident in HBM (device pointer, [n][dim] fp32 row-major); only enqueues"""
        n0 = self.count()
        rc = _lib.lib().zvec_hip_flat_append_fp32_dev(self._h, C.c_void_p(d_ptr), int(n), int(dim), int(dim if encode_dims is None else encode_dims),
                                                      float(threshold), C.c_void_p(d_keys_ptr) if d_keys_ptr else None,
                                                      C.c_void_p(stream) if stream else None)
        if rc == 0 and d_keys_ptr is None and n:
            self._keys_host.append(("range", n0, n0 + int(n)))
        return rc

    def _all_keys(self):
        parts = []
        for p in self._keys_host:
            if isinstance(p, tuple):
                parts.append(np.arange(p[1], p[2], dtype=np.uint64))
            else:
                parts.append(p)
        return np.concatenate(parts) if parts else np.zeros(0, np.uint64)

    def get_vector_by_id(self, pos):
        out = np.zeros(self.row_words, self.np_dtype)
        rc = _lib.lib().zvec_hip_flat_get_vector(self._h, int(pos), _np_ptr(out))
        return out if rc == 0 else None

    def get_vectors_by_ids(self, positions):
        pos = np.ascontiguousarray(positions, np.uint64)
        out = np.zeros((pos.size, self.row_words), self.np_dtype)
        _lib.check(_lib.lib().zvec_hip_flat_get_vectors(self._h, _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_flat_get_vectors")
        return out

    def _vectors_of_keys(self, keys):
        """stored rows of the documents with these keys (fetch_vector); key -> position through a sorted view of the keys"""
        allk = self._all_keys()
        order = np.argsort(allk, kind="stable")
        pos = order[np.searchsorted(allk[order], keys)]
        return self.get_vectors_by_ids(pos)

    def build_filter(self, doc_filter, ctx=None, d_out=None, stream=None):
        """DocFilter -> exclude bitset over this index's storage positions, built on the GPU.  Returns numpy
        uint64 words, or fills the device buffer `d_out` ((count+63)//64 uint64) and returns None."""
        n = self.count()
        words = None if d_out is not None else np.zeros((n + 63) // 64, np.uint64)
        desc = doc_filter._desc()
        rc = _lib.lib().zvec_hip_flat_build_filter(self._h, ctx._h if ctx else None, C.byref(desc),
                                                   C.c_void_p(d_out) if d_out is not None else _np_ptr(words),
                                                   int(d_out is not None), C.c_void_p(stream or 0))
        _lib.check(rc, "zvec_hip_flat_build_filter")
        return words

    def search_impl(self, query, count, ctx):
        """IndexRunner::search_impl(query, qmeta, count, context); query: [count][dim] fp32."""
        if ctx is None or (ctx.topk() == 0 and not ctx.group_by_search()):
            return IndexError_.InvalidArgument      # flat_searcher.cc:194-198
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.row_words:
            return IndexError_.InvalidArgument
        if ctx.group_by_search():
            return self._group_search(q, count, ctx, None)      # flat_streamer.cc:323-324
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        if ctx._doc_filter is not None:
            ex = self.build_filter(ctx._doc_filter, ctx)
        else:
            ex = ctx._exclude_for(self._all_keys()) if (ctx._filter_fn or ctx._exclude is not None) else None
        rc = _lib.lib().zvec_hip_flat_search(self._h, ctx._h, _np_ptr(q), count, k, ctx.threshold(),
                                             _np_ptr(ex), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    # brute force == the flat scan itself (flat_streamer.cc:304-344)
    search_bf_impl = search_impl

    def search_impl_fp32(self, queries, count, ctx, bin_threshold=0.0):
        """search_impl of a "Hamming" index of binary32 rows with fp32 queries ([count][dim]): BinaryReformer::transform on the GPU
        (every value against bin_threshold), then the search — results, filter and threshold as search_impl."""
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim != 2 or q.shape[0] != int(count):
            return IndexError_.InvalidArgument
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        if ctx._doc_filter is not None:
            ex = self.build_filter(ctx._doc_filter, ctx)
        else:
            ex = ctx._exclude_for(self._all_keys()) if (ctx._filter_fn or ctx._exclude is not None) else None
        rc = _lib.lib().zvec_hip_flat_search_fp32(self._h, ctx._h, _np_ptr(q), q.shape[1], float(bin_threshold), count, k, ctx.threshold(),
                                                  _np_ptr(ex), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    def search_fp32_dev(self, d_queries, dim, count, topk, d_out_keys, d_out_scores, d_out_counts, ctx, bin_threshold=0.0,
                        threshold=FLT_MAX, d_exclude=None, stream=None):
        """device-pointer form of search_impl_fp32 (async): all arguments are raw device pointers (ints)."""
        return _lib.lib().zvec_hip_flat_search_fp32_dev(
            self._h, ctx._h, C.c_void_p(d_queries), int(dim), float(bin_threshold), count, topk, threshold,
            C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts),
            C.c_void_p(stream) if stream else None)

    def _group_search(self, q, count, ctx, p_keys):
        """group_by_search_impl / group_by_search_p_keys_impl (flat_streamer.cc:391-483)"""
        if ctx._group_by is None:
            return IndexError_.InvalidArgument                  # "Invalid group-by function"
        allk = self._all_keys()
        of, ids = ctx._groups_for(allk)
        gnum, gk = ctx._group_num, ctx._group_topk
        groups = np.zeros((count, gnum), np.uint32)
        ngroups = np.zeros(count, np.uint32)
        keys = np.zeros((count, gnum, gk), np.uint64)
        scores = np.zeros((count, gnum, gk), np.float32)
        counts = np.zeros((count, gnum), np.uint32)
        L = _lib.lib()
        if p_keys is None:
            if ctx._doc_filter is not None:
                ex = self.build_filter(ctx._doc_filter, ctx)
            else:
                ex = ctx._exclude_for(allk) if (ctx._filter_fn or ctx._exclude is not None) else None
            rc = L.zvec_hip_flat_search_grouped(self._h, ctx._h, _np_ptr(q), count, _np_ptr(of), max(len(ids), 1), gnum, gk,
                                                ctx.threshold(), _np_ptr(ex), _np_ptr(groups), _np_ptr(ngroups), _np_ptr(keys),
                                                _np_ptr(scores), _np_ptr(counts))
        else:
            ids_l, offs = self._p_keys_positions(p_keys, ctx)
            rc = L.zvec_hip_flat_search_grouped_by_ids(self._h, ctx._h, _np_ptr(q), count, _np_ptr(ids_l), _np_ptr(offs), _np_ptr(of),
                                                       max(len(ids), 1), gnum, gk, ctx.threshold(), _np_ptr(ctx._exclude),
                                                       _np_ptr(groups), _np_ptr(ngroups), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_group_results(ids, groups, ngroups, keys, scores, counts, self._vectors_of_keys)
        return rc

    def _p_keys_positions(self, p_keys, ctx):
        """primary keys -> storage positions (unknown keys and keys the context's filter rejects are dropped)"""
        allk = self._all_keys()
        if getattr(self, "_key2pos_n", -1) != len(allk):
            self._key2pos = {int(k): i for i, k in enumerate(allk)}
            self._key2pos_n = len(allk)
        ids, offs = [], [0]
        for keys in p_keys:
            for key in keys:
                pos = self._key2pos.get(int(key))
                if pos is not None and not (ctx._filter_fn and ctx._filter_fn(int(key))):
                    ids.append(pos)
            offs.append(len(ids))
        return np.asarray(ids if ids else [0], np.uint32), np.asarray(offs, np.uint32)

    def search_bf_by_p_keys_impl(self, query, p_keys, count, ctx):
        """FlatStreamer::search_bf_by_p_keys_impl (flat_streamer.cc:346-389): p_keys[q] = primary keys query q
        is compared with; unknown keys are skipped; the context's filter applies per key."""
        if ctx is None or (ctx.topk() == 0 and not ctx.group_by_search()):
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.row_words or len(p_keys) != count:
            return IndexError_.InvalidArgument
        if ctx.group_by_search():
            return self._group_search(q, count, ctx, p_keys)    # flat_streamer.cc:365-366
        ids, offs = self._p_keys_positions(p_keys, ctx)
        return self._search_listed(q, ids, offs, count, ctx)

    def _search_listed(self, q, ids, offs, count, ctx):
        """query i against the storage positions ids[offs[i] .. offs[i + 1]) (zvec_hip_flat_search_by_ids)"""
        k = ctx.topk()
        keys_o = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        rc = _lib.lib().zvec_hip_flat_search_by_ids(self._h, ctx._h, _np_ptr(q), count, _np_ptr(ids), _np_ptr(offs), k,
                                                    ctx.threshold(), _np_ptr(ctx._exclude), _np_ptr(keys_o),
                                                    _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys_o, scores, counts, self._vectors_of_keys)
        return rc

    def search_by_positions_impl(self, query, positions, count, ctx):
        """search_bf_by_p_keys_impl for a caller that already holds storage positions: positions[i] = the rows query i is compared
        with (positions beyond the count and holes are skipped)."""
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.row_words or len(positions) != count:
            return IndexError_.InvalidArgument
        lens = [len(p) for p in positions]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        ids = np.concatenate([np.asarray(p, np.uint32).reshape(-1) for p in positions] + [np.zeros(0 if offs[-1] else 1, np.uint32)])
        return self._search_listed(q, np.ascontiguousarray(ids, np.uint32), offs, count, ctx)

    def batch_distance(self, query, positions, ctx=None):
        """IndexMetric::batch_distance: one query against the listed storage positions, scores in that order"""
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        pos = np.ascontiguousarray(positions, np.uint32)
        out = np.zeros(pos.size, np.float32)
        _lib.check(_lib.lib().zvec_hip_flat_batch_distance(self._h, ctx._h if ctx else None, _np_ptr(q), _np_ptr(pos), pos.size,
                                                           _np_ptr(out)), "zvec_hip_flat_batch_distance")
        return out

    def search_dev(self, d_queries, count, topk, d_out_keys, d_out_scores, d_out_counts, ctx,
                   threshold=FLT_MAX, d_exclude=None, stream=None):
        """device-pointer form (async): all arguments are raw device pointers (ints)."""
        return _lib.lib().zvec_hip_flat_search_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, threshold,
            C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys),
            C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)


    def set_shadow(self, enable=True, preselect=0):
        """half-width pre-selection (zvec_hip_flat_set_shadow): an fp16 twin of the rows present now is scanned for `preselect` rows
        per query, those are re-scored in fp32 and the result is certified; any later mutation of the store drops the twin"""
        _lib.check(_lib.lib().zvec_hip_flat_set_shadow(self._h, int(bool(enable)), int(preselect)), "zvec_hip_flat_set_shadow")

    def shadow_info(self):
        on, nbytes, err, norm = C.c_int(0), C.c_uint64(0), C.c_float(0), C.c_float(0)
        _lib.check(_lib.lib().zvec_hip_flat_shadow_info(self._h, C.byref(on), C.byref(nbytes), C.byref(err), C.byref(norm)),
                   "zvec_hip_flat_shadow_info")
        return {"enabled": bool(on.value), "bytes": int(nbytes.value), "max_row_error": float(err.value), "max_row_norm": float(norm.value)}

    def shadow_width(self, topk):
        """rows the next search with this k pre-selects per query (zvec_hip_flat_shadow_width; 0: no twin)"""
        n = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_flat_shadow_width(self._h, int(topk), C.byref(n)), "zvec_hip_flat_shadow_width")
        return int(n.value)

    def shadow_certify(self, d_queries, count, topk, d_out_keys, d_out_scores, d_out_counts, ctx, d_exclude=None, stream=None):
        """the second half of search_dev on a store with shadow rows: waits, re-runs the uncertified queries on the fp32 rows;
        returns how many were re-run"""
        n = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_flat_shadow_certify(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys),
            C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None, C.byref(n)),
            "zvec_hip_flat_shadow_certify")
        return int(n.value)


class HipFlatStreamer(_FlatBase):
    """stands where "FlatStreamer" is registered (flat_streamer.cc:486-489): mutable, add + search."""

    def add_impl(self, key, vec, ctx=None):
        return self.add_batch(np.asarray(vec, self.np_dtype).reshape(1, -1), np.array([key], np.uint64))

    INVALID_KEY = np.uint64(0xffffffffffffffff)          # kInvalidKey (flat_index_format.h:29)

    def add_with_id_impl(self, doc_id, vec, ctx=None):
        """IndexStreamer::add_with_id_impl (index_runner.h:483-487): what core_interface::Index::_dense_add calls"""
        return self.add_with_id_batch([doc_id], np.asarray(vec, self.np_dtype).reshape(1, -1))

    def add_with_id_batch(self, ids, vecs):
        """FlatStreamerEntity::add_vector_with_id row by row (flat_streamer_entity.cc:900-990): row ids[i] lives at
        storage position ids[i] under key ids[i]; gaps are padded with holes no search returns, an id below the count
        overwrites in place."""
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        ids = np.ascontiguousarray(ids, np.uint32)
        if vecs.ndim != 2 or vecs.shape[1] != self.row_words or ids.size != vecs.shape[0]:
            return IndexError_.InvalidArgument
        rc = _lib.lib().zvec_hip_flat_put(self._h, _np_ptr(ids), ids.size, _np_ptr(vecs), None)
        if rc == 0:
            keys = self._all_keys()
            n = self.count()
            if keys.size < n:
                keys = np.concatenate([keys, np.full(n - keys.size, self.INVALID_KEY, np.uint64)])
            keys[ids.astype(np.int64)] = ids.astype(np.uint64)
            self._keys_host = [keys]
        return rc

    def holes(self):
        c = C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_flat_holes(self._h, C.byref(c)), "zvec_hip_flat_holes")
        return int(c.value)


class _FlatFeatures:
    def load_features(self, features, count, column_major=False, batch_size=32, keys=None):
        """the features segment of a dumped flat index (FlatBuilder write_row_index / write_column_index layouts)"""
        fb = bytes(features)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        n0 = self.count()
        rc = _lib.lib().zvec_hip_flat_load_features(self._h, fb, len(fb), int(count), int(bool(column_major)), int(batch_size),
                                                    _np_ptr(k))
        if rc == 0:
            self._keys_host.append(np.arange(n0, n0 + int(count), dtype=np.uint64) if k is None else k.copy())
        return rc


class HipFlatSearcher(_FlatBase, _FlatFeatures):
    """stands where "FlatSearcher" is registered (flat_searcher.cc:247-250): load once, search."""

    def load(self, vecs, keys=None):
        return self.add_batch(vecs, keys)


class HipBinaryPreselectFlat:
    """Pre-select on sign bits, re-score on the fp32 rows: the usual deployment of a binary-quantised index, composed of two flat
    indexes that hold the same documents at the same storage positions —
      bits   a "Hamming" index of 32 * ceil(dim / 32) bits, fed through add_batch_fp32 / search_impl_fp32 (bit i = value i >= threshold),
      rows   an fp32 index of `dim` elements under `metric` ("SquaredEuclidean", "InnerProduct" or "Cosine"; `dim` is the index's
             element dimension, so Cosine rows and queries are the converted ones, norm slot included).
    search(queries, k, refine) takes min(n, k * refine) candidates per query from the bits and returns the k best of exactly those
    by the fp32 index's listed-rows search (search_by_positions_impl): no scoring and no kernel of its own, and the contract of
    that search for equal scores."""

    def __init__(self, dim, metric, device=0, threshold=0.0):
        if isinstance(metric, str):
            metric = metric_from_name(metric)
        if metric not in (METRIC_L2, METRIC_IP, METRIC_COSINE):
            raise ValueError("zvec_amd: HipBinaryPreselectFlat re-scores under SquaredEuclidean, InnerProduct or Cosine")
        self.dim = int(dim)
        self.threshold = float(threshold)
        self.bits = HipFlatSearcher((self.dim + 31) // 32 * 32, METRIC_HAMMING, device, "binary32")   # keys = storage positions
        self.rows = HipFlatSearcher(self.dim, metric, device)                                          # keys = the caller's
        self._bctx, self._rctx = self.bits.create_context(), self.rows.create_context()
        self.candidates = None        # of the last search: (positions uint32 [count][k * refine], counts [count])

    def count(self):
        return self.rows.count()

    def add_batch(self, rows, keys=None):
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            return IndexError_.InvalidArgument
        if self.bits.count() != self.rows.count():
            return IndexError_.Mismatch                     # (an earlier add_batch stored one half only)
        rc = self.bits.add_batch_fp32(rows, None, self.threshold)
        return rc if rc != 0 else self.rows.add_batch(rows, keys)

    def search(self, queries, k, refine=4):
        """returns (keys uint64 [count][k], scores fp32 [count][k], counts uint32 [count]), ascending by the fp32 score"""
        q = np.ascontiguousarray(queries, np.float32)
        n = self.count()
        if q.ndim != 2 or q.shape[1] != self.dim or k <= 0 or refine <= 0 or n == 0:
            raise ValueError("zvec_amd: HipBinaryPreselectFlat.search takes [count][dim] queries, k > 0, refine > 0 on a non-empty index")
        count = q.shape[0]
        self._bctx.set_topk(min(n, int(k) * int(refine)))
        _lib.check(self.bits.search_impl_fp32(q, count, self._bctx, self.threshold), "HipBinaryPreselectFlat: binary stage")
        pos, cnt = self._bctx.keys.astype(np.uint32), self._bctx.counts
        self.candidates = (pos, cnt)
        self._rctx.set_topk(int(k))
        _lib.check(self.rows.search_by_positions_impl(q, [pos[i, :int(cnt[i])] for i in range(count)], count, self._rctx),
                   "HipBinaryPreselectFlat: fp32 stage")
        return self._rctx.keys, self._rctx.scores, self._rctx.counts


class HipFlatSparseStreamer:
    """stands where "FlatSparseStreamer" / "FlatSparseSearcher" are registered (flat_sparse_streamer.cc, flat_sparse_searcher.cc):
    a flat index of sparse rows (zvec_hip_sparse_*) under metric "InnerProductSparse" (scores are minus the inner product) or
    "SquaredEuclideanSparse" (scores are squared distances over the union of the two index sets; include/zvec_hip.h, "Score"),
    readable as .metric.  A batch of rows or queries is CSR-like: counts[n],
    then the runs back to back in indices (uint32, strictly ascending inside a run) and values.  dtype "fp32" or "fp16"
    (IndexMeta::DT_FP32 / DT_FP16, inner_product_metric.cc:484-495): values go in and come out as numpy.float32 / numpy.float16,
    other float inputs are cast to that type; scores are fp32 either way."""

    MAX_COUNT = 4096            # PARAM_FLAT_SPARSE_MAX_DIM_SIZE (flat_sparse_utility.h:22)

    def __init__(self, device=0, dtype="fp32", metric="InnerProductSparse"):
        if metric not in _SPARSE_METRIC_NAMES:
            raise ValueError("zvec_amd: a sparse index serves %s, not %r" % (" and ".join(sorted(_SPARSE_METRIC_NAMES)), metric))
        self.device = device
        self.metric = metric
        self.dtype, self.np_dtype = _dtype_of(dtype)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_sparse_create_metric(self.dtype, _SPARSE_METRIC_NAMES[metric], device, C.byref(self._h)),
                   "zvec_hip_sparse_create_metric")
        self._keys_host = []      # for IndexFilter sweeps

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_sparse_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def create_context(self):
        return IndexContext(self.device)

    def count(self):
        n = C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_sparse_count(self._h, C.byref(n), None), "zvec_hip_sparse_count")
        return int(n.value)

    def element_count(self):
        n = C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_sparse_count(self._h, None, C.byref(n)), "zvec_hip_sparse_count")
        return int(n.value)

    def reserve(self, rows, elements):
        return _lib.lib().zvec_hip_sparse_reserve(self._h, int(rows), int(elements))

    def _runs(self, counts, indices, values):
        c = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        v = np.ascontiguousarray(values, self.np_dtype).reshape(-1)
        total = int(c.astype(np.uint64).sum())
        return (c, i, v) if i.size == total and v.size == total else None

    def add_batch(self, counts, indices, values, keys=None):
        runs = self._runs(counts, indices, values)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        if runs is None or (k is not None and k.size != runs[0].size):
            return IndexError_.InvalidArgument
        c, i, v = runs
        n0 = self.count()
        rc = _lib.lib().zvec_hip_sparse_append(self._h, _np_ptr(c), _np_ptr(i), _np_ptr(v), c.size, _np_ptr(k))
        if rc == 0 and c.size:
            self._keys_host.append(np.arange(n0, n0 + c.size, dtype=np.uint64) if k is None else k.copy())
        return rc

    INVALID_KEY = np.uint64(0xffffffffffffffff)          # kInvalidKey: what a hole is stored under

    def add_with_id_impl(self, doc_id, indices, values):
        """IndexStreamer::add_with_id_impl for one sparse document: what core_interface::Index::_sparse_add calls"""
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        return self.add_with_id_batch([doc_id], [i.size], i, values)

    def add_with_id_batch(self, ids, counts, indices, values, keys=None):
        """FlatSparseStreamerEntity::add_vector_with_id row by row (zvec_hip_sparse_put): row i goes to storage position ids[i]
        under key ids[i] (or keys[i]); a gap is padded with holes no search returns, an id below the count replaces the row,
        an id named twice keeps the later row.  All or nothing."""
        runs = self._runs(counts, indices, values)
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64).reshape(-1)
        if runs is None or ids.size != runs[0].size or (k is not None and k.size != ids.size):
            return IndexError_.InvalidArgument
        c, i, v = runs
        rc = _lib.lib().zvec_hip_sparse_put(self._h, _np_ptr(ids), _np_ptr(c), _np_ptr(i), _np_ptr(v), ids.size, _np_ptr(k))
        if rc == 0 and ids.size:
            self._put_keys(ids, ids.astype(np.uint64) if k is None else k, self.count())
        return rc

    def _put_keys(self, ids, keyvals, n):
        """the host key column after a put that left n rows: ONE array with room to grow, of which only the new positions (the
        invalid key) and the call's own are written, so that filling an index document by document costs the document, not the
        index.  Rows that came through add_batch since the last put are gathered into it once."""
        buf = getattr(self, "_key_buf", None)
        cur = self._keys_host
        if buf is not None and len(cur) == 1 and cur[0].base is buf:
            have = cur[0].size
        else:
            allk = self._all_keys()
            have = allk.size
            buf = np.empty(max(n, 2 * have, 16), np.uint64)
            buf[:have] = allk
        if n > buf.size:
            grown = np.empty(max(n, 2 * buf.size), np.uint64)
            grown[:have] = buf[:have]
            buf = grown
        buf[have:n] = self.INVALID_KEY
        _, first = np.unique(ids[::-1], return_index=True)          # the later row of an id wins: its last place in the call
        last = ids.size - 1 - first
        buf[ids[last].astype(np.int64)] = keyvals[last]
        self._key_buf = buf
        self._keys_host = [buf[:n]]

    def holes(self):
        c = C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_sparse_holes(self._h, C.byref(c)), "zvec_hip_sparse_holes")
        return int(c.value)

    def put_info(self):
        """the last successful add_with_id_batch (zvec_hip_sparse_put_info): route -1 none yet / 0 tail / 1 in place / 2 splice"""
        route, moved, chunk, ms = C.c_int(0), C.c_uint64(0), C.c_uint32(0), C.c_double(0.0)
        _lib.check(_lib.lib().zvec_hip_sparse_put_info(self._h, C.byref(route), C.byref(moved), C.byref(chunk), C.byref(ms)),
                   "zvec_hip_sparse_put_info")
        return {"route": int(route.value), "moved_elems": int(moved.value), "chunk_elems": int(chunk.value), "ms": float(ms.value)}

    def _all_keys(self):
        """the key of every storage position; a hole reports the invalid key"""
        if len(self._keys_host) == 1:
            return self._keys_host[0]                    # (no copy: read-only to its callers)
        return np.concatenate(self._keys_host) if self._keys_host else np.zeros(0, np.uint64)

    def get_vector_by_id(self, pos):
        """(indices, values) of the row at storage position `pos` as stored (a hole: empty), or None beyond the last row"""
        n = C.c_uint32(0)
        idx = np.zeros(self.MAX_COUNT, np.uint32)
        val = np.zeros(self.MAX_COUNT, self.np_dtype)
        rc = _lib.lib().zvec_hip_sparse_get_vector(self._h, int(pos), C.byref(n), _np_ptr(idx), _np_ptr(val))
        return (idx[:n.value].copy(), val[:n.value].copy()) if rc == 0 else None

    def set_inverted(self, enable=True):
        """inverted lists (zvec_hip_sparse_set_inverted): a term-major twin of the rows, InnerProductSparse only; while it is on,
        search_impl and search_dev walk the lists of the query's own indices instead of every stored row.  Built by the first search
        that needs it, rebuilt once by the first search after an append."""
        _lib.check(_lib.lib().zvec_hip_sparse_set_inverted(self._h, int(bool(enable))), "zvec_hip_sparse_set_inverted")

    def inverted_info(self):
        on, nbytes, terms, tile, builds = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_sparse_inverted_info(self._h, C.byref(on), C.byref(nbytes), C.byref(terms), C.byref(tile),
                                                            C.byref(builds)), "zvec_hip_sparse_inverted_info")
        return {"enabled": bool(on.value), "bytes": int(nbytes.value), "terms": int(terms.value), "tile_rows": int(tile.value),
                "builds": int(builds.value)}

    def inverted_export(self):
        """the inverted lists as they are held (zvec_hip_sparse_inverted_export; brought up to date first, as by a search):
        (terms uint32 [nterms], list_off uint64 [nterms + 1], ppos uint32 [elements], pval [elements] in the handle's dtype)"""
        L = _lib.lib()
        nt, ne = C.c_uint64(0), C.c_uint64(0)
        _lib.check(L.zvec_hip_sparse_inverted_export(self._h, None, 0, None, None, None, 0, C.byref(nt), C.byref(ne)),
                   "zvec_hip_sparse_inverted_export")
        terms, list_off = np.zeros(nt.value, np.uint32), np.zeros(nt.value + 1, np.uint64)
        ppos, pval = np.zeros(ne.value, np.uint32), np.zeros(ne.value, self.np_dtype)
        _lib.check(L.zvec_hip_sparse_inverted_export(self._h, _np_ptr(terms), nt.value, _np_ptr(list_off), _np_ptr(ppos), _np_ptr(pval),
                                                     ne.value, C.byref(nt), C.byref(ne)), "zvec_hip_sparse_inverted_export")
        return terms, list_off, ppos, pval

    def inverted_build_info(self):
        """the build that made the lists held now (zvec_hip_sparse_inverted_build_info): route 0 host / 1 device / -1 none yet"""
        route, passes, block, ms = C.c_int(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0.0)
        _lib.check(_lib.lib().zvec_hip_sparse_inverted_build_info(self._h, C.byref(route), C.byref(passes), C.byref(block), C.byref(ms)),
                   "zvec_hip_sparse_inverted_build_info")
        return {"route": int(route.value), "passes": int(passes.value), "block_elems": int(block.value), "ms": float(ms.value)}

    def search_impl(self, counts, indices, values, count, ctx):
        """search_impl(sparse_count, sparse_indices, sparse_query, qmeta, count, context) (flat_sparse_search.h:58-148)"""
        if ctx is None:
            return IndexError_.InvalidArgument
        if ctx.group_by_search():
            return IndexError_.Unsupported              # (not routed here: group_by_search_impl serves it when called directly)
        if ctx.topk() == 0:
            return IndexError_.InvalidArgument
        runs = self._runs(counts, indices, values)
        if runs is None or runs[0].size != int(count):
            return IndexError_.InvalidArgument
        c, i, v = runs
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        cnts = np.zeros(count, np.uint32)
        ex = ctx._exclude_for(self._all_keys()) if (ctx._filter_fn or ctx._exclude is not None) else None
        rc = _lib.lib().zvec_hip_sparse_search(self._h, ctx._h, _np_ptr(c), _np_ptr(i), _np_ptr(v), count, k, ctx.threshold(),
                                               _np_ptr(ex), _np_ptr(keys), _np_ptr(scores), _np_ptr(cnts))
        if rc == 0:
            ctx._set_results(keys, scores, cnts)
        return rc

    search_bf_impl = search_impl

    # primary keys -> storage positions, as FlatSparseEntity::search_p_keys does key by key (flat_sparse_entity.h:63-77): the dense
    # streamer's helper, which needs nothing of its owner but _all_keys()
    _p_keys_positions = _FlatBase._p_keys_positions

    def search_bf_by_p_keys_impl(self, counts, indices, values, p_keys, count, ctx):
        """FlatSparseStreamer::search_bf_by_p_keys_impl (flat_sparse_streamer.cc:324-349): p_keys[q] = the primary keys query q is
        compared with; unknown keys are skipped, the context's filter applies per key, its exclude bitset per position; a key
        listed twice is scored twice."""
        if ctx is None:
            return IndexError_.InvalidArgument
        if ctx.group_by_search():
            return IndexError_.Unsupported              # (not routed here: group_by_search_p_keys_impl serves it when called directly)
        if ctx.topk() == 0 or len(p_keys) != int(count):
            return IndexError_.InvalidArgument
        runs = self._runs(counts, indices, values)
        if runs is None or runs[0].size != int(count):
            return IndexError_.InvalidArgument
        c, i, v = runs
        ids, offs = self._p_keys_positions(p_keys, ctx)
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        cnts = np.zeros(count, np.uint32)
        rc = _lib.lib().zvec_hip_sparse_search_by_ids(self._h, ctx._h, _np_ptr(c), _np_ptr(i), _np_ptr(v), count, _np_ptr(ids),
                                                      _np_ptr(offs), k, ctx.threshold(), _np_ptr(ctx._exclude), _np_ptr(keys),
                                                      _np_ptr(scores), _np_ptr(cnts))
        if rc == 0:
            ctx._set_results(keys, scores, cnts)
        return rc

    def _group_search(self, counts, indices, values, count, ctx, p_keys):
        if ctx is None or not ctx.group_by_search() or ctx._group_topk <= 0:
            return IndexError_.InvalidArgument
        if ctx._group_by is None:
            return IndexError_.InvalidArgument                  # "Invalid group-by function"
        runs = self._runs(counts, indices, values)
        if runs is None or runs[0].size != int(count) or (p_keys is not None and len(p_keys) != int(count)):
            return IndexError_.InvalidArgument
        c, i, v = runs
        allk = self._all_keys()
        of, ids = ctx._groups_for(allk)
        gnum, gk = ctx._group_num, ctx._group_topk
        groups = np.zeros((count, gnum), np.uint32)
        ngroups = np.zeros(count, np.uint32)
        keys = np.zeros((count, gnum, gk), np.uint64)
        scores = np.zeros((count, gnum, gk), np.float32)
        cnts = np.zeros((count, gnum), np.uint32)
        if len(of) == 0:
            of = np.zeros(1, np.uint32)                         # (an empty index: nothing of it is read)
        L = _lib.lib()
        if p_keys is None:
            ex = ctx._exclude_for(allk) if (ctx._filter_fn or ctx._exclude is not None) else None
            rc = L.zvec_hip_sparse_search_grouped(self._h, ctx._h, _np_ptr(c), _np_ptr(i), _np_ptr(v), count, _np_ptr(of),
                                                  max(len(ids), 1), gnum, gk, ctx.threshold(), _np_ptr(ex), _np_ptr(groups),
                                                  _np_ptr(ngroups), _np_ptr(keys), _np_ptr(scores), _np_ptr(cnts))
        else:
            ids_l, offs = self._p_keys_positions(p_keys, ctx)
            rc = L.zvec_hip_sparse_search_grouped_by_ids(self._h, ctx._h, _np_ptr(c), _np_ptr(i), _np_ptr(v), count, _np_ptr(ids_l),
                                                         _np_ptr(offs), _np_ptr(of), max(len(ids), 1), gnum, gk, ctx.threshold(),
                                                         _np_ptr(ctx._exclude), _np_ptr(groups), _np_ptr(ngroups), _np_ptr(keys),
                                                         _np_ptr(scores), _np_ptr(cnts))
        if rc == 0:
            ctx._set_group_results(ids, groups, ngroups, keys, scores, cnts)
        return rc

    def group_by_search_impl(self, counts, indices, values, count, ctx):
        """the group-by branch of the sparse search (flat_sparse_search.h:77-117 -> FlatSparseEntity::search_group,
        flat_sparse_entity.h:79-103; ConvertGroupMapToResult, flat_sparse_search.h:23-53) through
        zvec_hip_sparse_search_grouped: the context's group parameters and group_by function, its filter / exclude bitset as in
        search_impl; results in ctx.group_result(q).  Called directly: search_impl itself still answers Unsupported under a group
        context."""
        return self._group_search(counts, indices, values, count, ctx, None)

    def group_by_search_p_keys_impl(self, counts, indices, values, p_keys, count, ctx):
        """the same over listed primary keys (FlatSparseEntity::search_group_p_keys, flat_sparse_entity.h:105-128) through
        zvec_hip_sparse_search_grouped_by_ids; keys are mapped and filtered as in search_bf_by_p_keys_impl, which itself still
        answers Unsupported under a group context."""
        return self._group_search(counts, indices, values, count, ctx, p_keys)

    def batch_distance(self, indices, values, positions, ctx=None):
        """IndexMetric::batch_distance: one sparse query against the listed storage positions, fp32 scores in that order (+inf for a
        position beyond the rows)"""
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        v = np.ascontiguousarray(values, self.np_dtype).reshape(-1)
        if i.size != v.size:
            raise ValueError("zvec_amd: a sparse query needs as many values as indices")
        pos = np.ascontiguousarray(positions, np.uint32).reshape(-1)
        out = np.zeros(pos.size, np.float32)
        _lib.check(_lib.lib().zvec_hip_sparse_batch_distance(self._h, ctx._h if ctx else None, i.size, _np_ptr(i), _np_ptr(v),
                                                             _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_sparse_batch_distance")
        return out

    def search_dev(self, counts, d_indices, d_values, count, topk, d_out_keys, d_out_scores, d_out_counts, ctx,
                   threshold=FLT_MAX, d_exclude=None, stream=None):
        """device-pointer form (async): `counts` is a HOST array (the host cuts the batch into query blocks), everything else raw
        device pointers (ints).  d_values holds elements of the index's value type: halves (2 bytes each) for an fp16 index."""
        c = np.ascontiguousarray(counts, np.uint32).reshape(-1)
        if c.size != int(count):
            return IndexError_.InvalidArgument
        return _lib.lib().zvec_hip_sparse_search_dev(
            self._h, ctx._h, _np_ptr(c), C.c_void_p(d_indices), C.c_void_p(d_values), count, topk, threshold,
            C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys), C.c_void_p(d_out_scores),
            C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)

    # ---- rows and queries that are torch tensors on the index's device (include/zvec_hip.h, "Rows and queries from device memory") ----
    def _keys_dev(self, keys, n):
        return None if keys is None else _torch_array(keys, self.device, "keys", _torch_words(64), n)

    def _stored_dev(self, n0, n, keys):
        if n:
            self._keys_host.append(np.arange(n0, n0 + n, dtype=np.uint64) if keys is None
                                   else keys.cpu().numpy().view(np.uint64).copy())

    def add_csr_dev(self, counts, indices, values, keys=None):
        """add_batch with every array a torch tensor on the index's device (zvec_hip_sparse_append_dev): counts / indices int32 or
        uint32, values of the index's type, keys int64 or uint64.  Validated on the device; all or nothing.  Runs on torch's
        current stream and returns with the rows stored.  A CPU tensor or a wrong dtype raises ValueError."""
        c = _torch_array(counts, self.device, "counts", _torch_words(32))
        i = _torch_array(indices, self.device, "indices", _torch_words(32))
        v = _torch_array(values, self.device, "values", (_torch_float(self.dtype),), i.numel())
        k = self._keys_dev(keys, c.numel())
        n0 = self.count()
        rc = _lib.lib().zvec_hip_sparse_append_dev(self._h, _torch_ptr(c), _torch_ptr(i), _torch_ptr(v), c.numel(), i.numel(),
                                                   _torch_ptr(k), _torch_stream(self.device))
        if rc == 0:
            self._stored_dev(n0, c.numel(), k)
        return rc

    def put_dev(self, ids, counts, indices, values, keys=None, stream=None):
        """add_with_id_batch with every array a torch tensor on the index's device (zvec_hip_sparse_put_dev): ids / counts /
        indices int32 or uint32, values of the index's type, keys int64 or uint64.  Validated on the device; the pairs and the
        keys stay there; all or nothing.  Runs on `stream` (a torch stream; None: torch's current one) and returns the status,
        with the rows stored when it is 0.  A CPU tensor or a wrong dtype raises ValueError."""
        c = _torch_array(counts, self.device, "counts", _torch_words(32))
        d = _torch_array(ids, self.device, "ids", _torch_words(32), c.numel())
        i = _torch_array(indices, self.device, "indices", _torch_words(32))
        v = _torch_array(values, self.device, "values", (_torch_float(self.dtype),), i.numel())
        k = self._keys_dev(keys, c.numel())
        if stream is None:
            s = _torch_stream(self.device)
        else:
            s = C.c_void_p(stream.cuda_stream)
            if not s.value:
                stream.synchronize()                         # (the default stream, as _torch_stream treats it)
        rc = _lib.lib().zvec_hip_sparse_put_dev(self._h, _torch_ptr(d), _torch_ptr(c), _torch_ptr(i), _torch_ptr(v), c.numel(),
                                                i.numel(), _torch_ptr(k), s)
        if rc == 0 and c.numel():
            h_ids = d.cpu().numpy().view(np.uint32)
            self._put_keys(h_ids, h_ids.astype(np.uint64) if k is None else k.cpu().numpy().view(np.uint64), self.count())
        return rc

    def add_dense(self, matrix, keys=None):
        """the non-zeros of every row of a dense [n, dim] torch tensor of the index's type on its device, column j as index j
        (zvec_hip_sparse_append_dense_dev).  Rows may be `stride(0)` elements apart (a column slice of a wider matrix); columns
        that are not adjacent are copied first.  -0.0 counts as zero; a row with more than 4096 non-zeros refuses the whole call."""
        m, ld = _torch_matrix(matrix, self.device, _torch_float(self.dtype))
        k = self._keys_dev(keys, m.shape[0])
        n0 = self.count()
        rc = _lib.lib().zvec_hip_sparse_append_dense_dev(self._h, _torch_ptr(m), m.shape[0], m.shape[1], ld, _torch_ptr(k),
                                                         _torch_stream(self.device))
        if rc == 0:
            self._stored_dev(n0, m.shape[0], k)
        return rc

    def search_dense(self, matrix, topk, threshold=None, exclude=None, ctx=None):
        """zvec_hip_sparse_search_dense_dev: the rows of a dense [count, dim] torch tensor as queries.  Returns torch tensors on the
        device, (keys int64 [count, topk] holding the uint64 keys' bits, scores float32 [count, topk], counts int32 [count]),
        enqueued on torch's current stream.  exclude: a device tensor of 64-bit words, bit i = storage position i."""
        import torch
        m, ld = _torch_matrix(matrix, self.device, _torch_float(self.dtype))
        ex = None if exclude is None else _torch_array(exclude, self.device, "exclude", _torch_words(64))
        count, k = m.shape[0], int(topk)
        keys = torch.zeros((count, k), dtype=torch.int64, device=m.device)
        scores = torch.zeros((count, k), dtype=torch.float32, device=m.device)
        cnts = torch.zeros(count, dtype=torch.int32, device=m.device)
        if ctx is None:
            ctx = getattr(self, "_dense_ctx", None) or IndexContext(self.device)
            self._dense_ctx = ctx
        stream = _torch_stream(self.device)
        _lib.check(_lib.lib().zvec_hip_sparse_search_dense_dev(
            self._h, ctx._h, _torch_ptr(m), count, m.shape[1], ld, k, FLT_MAX if threshold is None else threshold,
            _torch_ptr(ex), _torch_ptr(keys), _torch_ptr(scores), _torch_ptr(cnts), stream), "zvec_hip_sparse_search_dense_dev")
        if not stream.value:
            ctx.synchronize()
        return keys, scores, cnts

    def ingest_info(self):
        """the last successful add_csr_dev / add_dense (zvec_hip_sparse_ingest_info): route -1 none yet / 0 CSR / 1 dense"""
        route, elems, cols, ms = C.c_int(0), C.c_uint64(0), C.c_uint32(0), C.c_double(0.0)
        _lib.check(_lib.lib().zvec_hip_sparse_ingest_info(self._h, C.byref(route), C.byref(elems), C.byref(cols), C.byref(ms)),
                   "zvec_hip_sparse_ingest_info")
        return {"route": int(route.value), "elements": int(elems.value), "slice_cols": int(cols.value), "ms": float(ms.value)}


def _torch_words(bits):
    import torch
    names = ("int%d" % bits, "uint%d" % bits)           # (the same bits either way; older torch has no unsigned types)
    return tuple(getattr(torch, n) for n in names if hasattr(torch, n))


def _torch_float(dt):
    import torch
    return torch.float16 if dt == DT_FP16 else torch.float32


def _torch_array(t, device, what, dtypes, numel=None):
    """a torch tensor on cuda:`device` of one of `dtypes` (and of `numel` elements) as a contiguous 1-d one, or ValueError"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != device:
        raise ValueError("zvec_amd: %s must be a torch tensor on cuda:%d" % (what, device))
    if t.dtype not in dtypes:
        raise ValueError("zvec_amd: %s must be %s, not %s" % (what, " or ".join(str(d) for d in dtypes), t.dtype))
    if numel is not None and t.numel() != numel:
        raise ValueError("zvec_amd: %s must hold %d elements, not %d" % (what, numel, t.numel()))
    return t.contiguous().reshape(-1)


def _torch_matrix(t, device, dtype):
    """a 2-d torch tensor on cuda:`device` of `dtype` -> (the tensor with adjacent columns, its row stride in elements), or ValueError"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != device:
        raise ValueError("zvec_amd: the matrix must be a torch tensor on cuda:%d" % device)
    if t.dtype != dtype:
        raise ValueError("zvec_amd: the matrix must be %s, not %s" % (dtype, t.dtype))
    if t.dim() != 2:
        raise ValueError("zvec_amd: the matrix must have two dimensions")
    n, dim = t.shape
    if (dim > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < dim):
        t = t.contiguous()
    return t, max(int(t.stride(0)) if n > 1 else 0, int(dim))


def _torch_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _torch_stream(device):
    """torch's current stream as the library takes one.  The default stream has no handle to pass: it is drained instead (the
    tensors are complete) and the library works on a stream of its own, which the callers below drain before they return."""
    import torch
    s = torch.cuda.current_stream(device)
    if not s.cuda_stream:
        s.synchronize()
    return C.c_void_p(s.cuda_stream)


def sparse_from_dense(matrix, ctx=None):
    """zvec_hip_sparse_from_dense_dev: a dense [n, dim] float32 or float16 torch tensor on a GPU -> (counts int32 [n], indices int32
    [elements], values [elements] of the matrix's type), torch tensors on the same device: the non-zeros of every row in column
    order, bit for bit (-0.0 counts as zero).  A size query first, then the fill, both on torch's current stream."""
    import torch
    if not isinstance(matrix, torch.Tensor) or not matrix.is_cuda:
        raise ValueError("zvec_amd: the matrix must be a torch tensor on a GPU")
    if matrix.dtype not in (torch.float32, torch.float16):
        raise ValueError("zvec_amd: the matrix must be float32 or float16, not %s" % matrix.dtype)
    device = matrix.device.index
    m, ld = _torch_matrix(matrix, device, matrix.dtype)
    ctx = ctx or IndexContext(device)
    dt = DT_FP16 if m.dtype == torch.float16 else DT_FP32
    n, dim = m.shape
    counts = torch.zeros(n, dtype=torch.int32, device=m.device)
    indices = torch.zeros(0, dtype=torch.int32, device=m.device)
    values = torch.zeros(0, dtype=m.dtype, device=m.device)
    if n == 0:
        return counts, indices, values
    total = C.c_uint64(0)
    L = _lib.lib()
    _lib.check(L.zvec_hip_sparse_from_dense_dev(ctx._h, dt, _torch_ptr(m), n, dim, ld, _torch_ptr(counts), None, None, 0,
                                                C.byref(total), _torch_stream(device)), "zvec_hip_sparse_from_dense_dev")
    if total.value:
        indices = torch.zeros(total.value, dtype=torch.int32, device=m.device)
        values = torch.zeros(total.value, dtype=m.dtype, device=m.device)
        stream = _torch_stream(device)
        _lib.check(L.zvec_hip_sparse_from_dense_dev(ctx._h, dt, _torch_ptr(m), n, dim, ld, _torch_ptr(counts), _torch_ptr(indices),
                                                    _torch_ptr(values), total.value, C.byref(total), stream),
                   "zvec_hip_sparse_from_dense_dev")
        if not stream.value:
            ctx.synchronize()
    return counts, indices, values


class HipIVFSearcher:
    """stands where "IVFSearcher"/"IVFStreamer" are registered (ivf_searcher.cc:183-250)."""

    def __init__(self, dim, metric=METRIC_L2, device=0, scan_ratio=0.1, brute_force_threshold=1000, dtype="fp32"):
        if isinstance(metric, str):
            metric = metric_from_name(metric)
        self.dim = int(dim)
        self.metric = metric
        self.device = device
        self.dtype, self.np_dtype = _dtype_of(dtype)
        # IVFSearcherContext defaults (ivf_searcher_context.h:211-213)
        self.scan_ratio = float(scan_ratio)
        self.brute_force_threshold = int(brute_force_threshold)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_ivf_create(self.dim, self.dtype, metric, device, C.byref(self._h)),
                   "zvec_hip_ivf_create")
        self._list_keys = None    # keys in list order (filter sweeps)
        self._orig_keys = None    # keys per original row (build)
        self.total_count = 0

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_ivf_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def create_context(self):
        return IndexContext(self.device)

    def set_shard(self, shard, nshards):
        return _lib.lib().zvec_hip_ivf_keep_shard(self._h, shard, nshards)

    def load(self, centroids, list_offsets, vecs, keys=None):
        centroids = np.ascontiguousarray(centroids, self.np_dtype)
        lo = np.ascontiguousarray(list_offsets, np.uint64)
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_ivf_load(self._h, _np_ptr(centroids), centroids.shape[0], _np_ptr(lo),
                                          _np_ptr(vecs), _np_ptr(k))
        if rc == 0:
            self.total_count = int(lo[-1])
            self._orig_keys = k
            self._list_keys = None
        return rc

    def load_segments(self, inverted_header, inverted_meta, inverted_body, keys, centroids):
        """IVFSearcher::load from the raw segment payloads of a dumped reference index (bytes objects: "ivf.inverted_header",
        "ivf.inverted_meta", "ivf.inverted_body", "hc.keys") + the centroid rows; see zvec_hip_ivf_load_segments."""
        cent = np.ascontiguousarray(centroids, self.np_dtype)
        hb, mb, bb, kb = bytes(inverted_header), bytes(inverted_meta), bytes(inverted_body), bytes(keys)
        rc = _lib.lib().zvec_hip_ivf_load_segments(self._h, hb, len(hb), mb, len(mb), bb, len(bb), kb, len(kb), _np_ptr(cent))
        if rc == 0:
            self.total_count = len(kb) // 8
            self._orig_keys = np.frombuffer(kb, np.uint64, self.total_count).copy()
            self._list_keys = None
        return rc

    def build(self, vecs, nlist, keys=None, kmeans_iters=10, sample_per_list=256, seed=20260320):
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_ivf_build(self._h, _np_ptr(vecs), vecs.shape[0], _np_ptr(k), nlist,
                                           kmeans_iters, sample_per_list, seed)
        if rc == 0:
            self.total_count = vecs.shape[0]
            self._orig_keys = k
            self._list_keys = None
        return rc

    def build_dev(self, d_vecs, n, nlist, keys=None, kmeans_iters=10, sample_per_list=256, seed=20260320,
                  stream=None):
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_ivf_build_dev(self._h, C.c_void_p(d_vecs), int(n), _np_ptr(k), nlist,
                                               kmeans_iters, sample_per_list, seed,
                                               C.c_void_p(stream) if stream else None)
        if rc == 0:
            self.total_count = int(n)
            self._orig_keys = k
            self._list_keys = None
        return rc

    # ---- streamed build (IVFBuilder train / label / dump as separate steps; see include/zvec_hip.h) ----
    def train_dev(self, d_sample, n_sample, nlist, kmeans_iters=10, seed=20260320, stream=None):
        return _lib.lib().zvec_hip_ivf_train_dev(self._h, C.c_void_p(d_sample), int(n_sample), int(nlist), int(kmeans_iters),
                                                 int(seed), C.c_void_p(stream) if stream else None)

    def set_centroids(self, centroids):
        cent = np.ascontiguousarray(centroids, self.np_dtype)
        return _lib.lib().zvec_hip_ivf_set_centroids(self._h, _np_ptr(cent), cent.shape[0])

    def get_centroids(self):
        nl = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_ivf_get_centroids(self._h, None, C.byref(nl)), "zvec_hip_ivf_get_centroids")
        cent = np.zeros((int(nl.value), self.dim), self.np_dtype)
        _lib.check(_lib.lib().zvec_hip_ivf_get_centroids(self._h, _np_ptr(cent), None), "zvec_hip_ivf_get_centroids")
        return cent

    def label_dev(self, d_rows, n, d_labels, stream=None):
        """d_labels: device uint32[n]; complete when the call returns."""
        return _lib.lib().zvec_hip_ivf_label_dev(self._h, C.c_void_p(d_rows), int(n), C.c_void_p(d_labels),
                                                 C.c_void_p(stream) if stream else None)

    def begin_lists(self, list_sizes):
        sz = np.ascontiguousarray(list_sizes, np.uint32)
        rc = _lib.lib().zvec_hip_ivf_begin_lists(self._h, _np_ptr(sz))
        if rc == 0:
            self.total_count = int(sz.astype(np.uint64).sum())
            self._orig_keys = None
            self._list_keys = None
            self._streamed_keys = False
        return rc

    def add_dev(self, d_rows, n, labels, first_row, keys=None, stream=None):
        lab = np.ascontiguousarray(labels, np.uint32)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        if k is not None:
            self._streamed_keys = True     # explicit keys arrive per chunk: keys_in_list_order() is not tracked for them
        return _lib.lib().zvec_hip_ivf_add_dev(self._h, C.c_void_p(d_rows), int(n), _np_ptr(lab), _np_ptr(k), int(first_row),
                                               C.c_void_p(stream) if stream else None)

    def end_lists(self):
        return _lib.lib().zvec_hip_ivf_end_lists(self._h)

    def list_owners(self):
        own = np.zeros(self.info()[1], np.uint32)
        _lib.check(_lib.lib().zvec_hip_ivf_list_owners(self._h, _np_ptr(own)), "zvec_hip_ivf_list_owners")
        return own

    def info(self):
        n = C.c_uint64(0)
        nl = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_ivf_info(self._h, C.byref(n), C.byref(nl)), "zvec_hip_ivf_info")
        return int(n.value), int(nl.value)

    def export(self):
        n, nlist = self.info()
        cent = np.zeros((nlist, self.dim), self.np_dtype)
        lo = np.zeros(nlist + 1, np.uint64)
        rows = np.zeros(n, np.uint64)
        _lib.check(_lib.lib().zvec_hip_ivf_export(self._h, _np_ptr(cent), _np_ptr(lo), _np_ptr(rows)),
                   "zvec_hip_ivf_export")
        return cent, lo, rows

    def get_vector_by_id(self, list_pos):
        out = np.zeros(self.dim, self.np_dtype)
        rc = _lib.lib().zvec_hip_ivf_get_vector(self._h, int(list_pos), _np_ptr(out))
        return out if rc == 0 else None

    def get_vectors_by_ids(self, list_positions):
        pos = np.ascontiguousarray(list_positions, np.uint64)
        out = np.zeros((pos.size, self.dim), self.np_dtype)
        _lib.check(_lib.lib().zvec_hip_ivf_get_vectors(self._h, _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_ivf_get_vectors")
        return out

    def _vectors_of_keys(self, keys):
        lk = self.keys_in_list_order()
        order = np.argsort(lk, kind="stable")
        return self.get_vectors_by_ids(order[np.searchsorted(lk[order], keys)])

    # IVFSearcherContext::update (ivf_searcher_context.h:61-79)
    def probe_params(self, ctx=None):
        """nprobe / max_scan_count from the searcher's defaults, or from what the context's update(params) set"""
        ratio = self.scan_ratio if ctx is None or ctx._scan_ratio is None else ctx._scan_ratio
        bft = self.brute_force_threshold if ctx is None or ctx._bf_threshold is None else ctx._bf_threshold
        return ivf_probe_params(self.info()[1], self.total_count, ratio, bft)

    def set_nprobe(self, nprobe, exact=True):
        """boundary A's `nprobe` as patches/boundary_a.diff hands it to the searcher context: scan_ratio = nprobe / nlist;
        exact=True also sets brute_force_threshold = N - 1, which makes every query probe exactly nprobe lists
        (max_scan_count then never cuts the probe loop short)."""
        self.scan_ratio = float(np.float32(nprobe) / np.float32(max(self.info()[1], 1)))
        if exact:
            self.brute_force_threshold = max(self.total_count - 1, 0)

    def keys_in_list_order(self):
        """key of every dense list-order position (what IVFEntity::get_keys reads, ivf_entity.cc:612)."""
        if self._list_keys is None:
            _, _, rows = self.export()
            self._list_keys = rows if self._orig_keys is None else self._orig_keys[rows.astype(np.int64)]
        return self._list_keys

    def build_filter(self, doc_filter, ctx=None, d_out=None, stream=None):
        """DocFilter -> exclude bitset over list-order positions (see _FlatBase.build_filter)."""
        n = self.info()[0]
        words = None if d_out is not None else np.zeros((n + 63) // 64, np.uint64)
        desc = doc_filter._desc()
        rc = _lib.lib().zvec_hip_ivf_build_filter(self._h, ctx._h if ctx else None, C.byref(desc),
                                                  C.c_void_p(d_out) if d_out is not None else _np_ptr(words),
                                                  int(d_out is not None), C.c_void_p(stream or 0))
        _lib.check(rc, "zvec_hip_ivf_build_filter")
        return words

    def _exclude(self, ctx):
        if ctx._doc_filter is not None:
            return self.build_filter(ctx._doc_filter, ctx)
        if ctx._exclude is not None:
            return ctx._exclude
        if ctx._filter_fn is None:
            return None
        return ctx._exclude_for(self.keys_in_list_order())

    def search_impl(self, query, count, ctx):
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument      # ivf_searcher.cc:197-200
        bft = self.brute_force_threshold if ctx._bf_threshold is None else ctx._bf_threshold
        if self.total_count <= bft:
            return self.search_bf_impl(query, count, ctx)   # ivf_searcher.cc:188-190
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.dim:
            return IndexError_.InvalidArgument
        k = ctx.topk()
        nprobe, max_scan = self.probe_params(ctx)
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        ex = self._exclude(ctx)
        rc = _lib.lib().zvec_hip_ivf_search(self._h, ctx._h, _np_ptr(q), count, k, ctx.threshold(), nprobe,
                                            max_scan, _np_ptr(ex), _np_ptr(keys), _np_ptr(scores),
                                            _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    def search_bf_impl(self, query, count, ctx):
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.dim:
            return IndexError_.InvalidArgument
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        ex = self._exclude(ctx)
        rc = _lib.lib().zvec_hip_ivf_search_bf(self._h, ctx._h, _np_ptr(q), count, k, ctx.threshold(),
                                               _np_ptr(ex), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    def search_dev(self, d_queries, count, topk, nprobe, max_scan, d_out_keys, d_out_scores, d_out_counts,
                   ctx, threshold=FLT_MAX, d_exclude=None, stream=None):
        return _lib.lib().zvec_hip_ivf_search_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, threshold, nprobe, max_scan,
            C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys), C.c_void_p(d_out_scores),
            C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)

    def set_shadow(self, enable=True, preselect=0):
        """half-width pre-selection (zvec_hip_ivf_set_shadow): an fp16 twin of the fp32 lists is scanned for `preselect` rows per
        query, those are re-scored in fp32 and the result is certified; uncertified queries are re-run on the fp32 lists"""
        _lib.check(_lib.lib().zvec_hip_ivf_set_shadow(self._h, int(bool(enable)), int(preselect)), "zvec_hip_ivf_set_shadow")

    def shadow_info(self):
        on, nbytes, err, norm = C.c_int(0), C.c_uint64(0), C.c_float(0), C.c_float(0)
        _lib.check(_lib.lib().zvec_hip_ivf_shadow_info(self._h, C.byref(on), C.byref(nbytes), C.byref(err), C.byref(norm)),
                   "zvec_hip_ivf_shadow_info")
        return {"enabled": bool(on.value), "bytes": int(nbytes.value), "max_row_error": float(err.value), "max_row_norm": float(norm.value)}

    def shadow_width(self, topk):
        """rows the next search with this k pre-selects per query (zvec_hip_ivf_shadow_width; 0: no twin)"""
        n = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_ivf_shadow_width(self._h, int(topk), C.byref(n)), "zvec_hip_ivf_shadow_width")
        return int(n.value)

    def shadow_certify(self, d_queries, count, topk, nprobe, max_scan, d_out_keys, d_out_scores, d_out_counts, ctx,
                       d_exclude=None, stream=None):
        """the second half of search_dev on an index with shadow lists: waits, re-runs the uncertified queries on the fp32 lists;
        returns how many were re-run"""
        n = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_ivf_shadow_certify(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, nprobe, max_scan, C.c_void_p(d_exclude) if d_exclude else None,
            C.c_void_p(d_out_keys), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None,
            C.byref(n)), "zvec_hip_ivf_shadow_certify")
        return int(n.value)

    def coarse_dev(self, d_queries, count, nprobe, d_probe_idx, d_probe_cnt, ctx, stream=None):
        """the coarse pass alone (zvec_hip_ivf_coarse_dev): probe lists [count][min(nprobe, nlist)] u32 + [count] u32, device pointers"""
        return _lib.lib().zvec_hip_ivf_coarse_dev(self._h, ctx._h, C.c_void_p(d_queries), count, nprobe, C.c_void_p(d_probe_idx),
                                                  C.c_void_p(d_probe_cnt), C.c_void_p(stream) if stream else None)

    def search_probes_dev(self, d_queries, count, topk, nprobe, max_scan, d_probe_idx, d_probe_cnt, d_out_keys, d_out_scores,
                          d_out_counts, ctx, threshold=FLT_MAX, d_exclude=None, stream=None):
        """zvec_hip_ivf_search_dev without its coarse pass: plans from the given probe lists (zvec_hip_ivf_search_probes_dev)"""
        return _lib.lib().zvec_hip_ivf_search_probes_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, threshold, nprobe, max_scan, C.c_void_p(d_probe_idx),
            C.c_void_p(d_probe_cnt), C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys), C.c_void_p(d_out_scores),
            C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)

    def last_stats(self, ctx, count):
        scanned = np.zeros(count, np.uint32)
        probes = np.zeros(count, np.uint32)
        _lib.check(_lib.lib().zvec_hip_ivf_last_stats(self._h, ctx._h, count, _np_ptr(scanned), _np_ptr(probes)),
                   "zvec_hip_ivf_last_stats")
        return scanned, probes


# "IVFStreamer" (what the product instantiates, indexes/ivf_index.cc:38-39) is a read-only operator over a dumped index
# in the reference too (ivf_streamer.h:28-85): same class
HipIVFStreamer = HipIVFSearcher


class HipHammingIVFSearcher:
    """Binary rows under the Hamming metric through inverted lists (zvec_hip_bivf_*): what IVFStreamer / IVFSearcher are over a
    binary meta (ivf_streamer.cc:183-250 never looks at the data type).  Shaped like HipIVFSearcher; dim counts bits, rows are
    dim // 32 uint32 ("binary32") or dim // 64 uint64 ("binary64") words."""

    def __init__(self, dim, device=0, dtype="binary32", scan_ratio=0.1, brute_force_threshold=1000):
        self.dim = int(dim)
        self.metric = METRIC_HAMMING
        self.device = device
        self.dtype, self.np_dtype = _dtype_of(dtype)
        self.row_words = _row_words(self.dim, self.dtype)
        self.scan_ratio = float(scan_ratio)
        self.brute_force_threshold = int(brute_force_threshold)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_bivf_create(self.dim, self.dtype, device, C.byref(self._h)), "zvec_hip_bivf_create")
        self._list_keys = None
        self._orig_keys = None
        self.total_count = 0

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_bivf_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def create_context(self):
        return IndexContext(self.device)

    def _loaded(self, rc, n, keys):
        if rc == 0:
            self.total_count = int(n)
            self._orig_keys = keys
            self._list_keys = None
        return rc

    def load(self, centroids, list_offsets, rows, keys=None):
        cent = np.ascontiguousarray(centroids, self.np_dtype)
        lo = np.ascontiguousarray(list_offsets, np.uint64)
        rows = np.ascontiguousarray(rows, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        if cent.ndim != 2 or cent.shape[1] != self.row_words or lo.size != cent.shape[0] + 1 or rows.size != int(lo[-1]) * self.row_words:
            return IndexError_.InvalidArgument
        rc = _lib.lib().zvec_hip_bivf_load(self._h, _np_ptr(cent), cent.shape[0], _np_ptr(lo), _np_ptr(rows), _np_ptr(k))
        # (keys are given per list-order position: keys_in_list_order is them, or the positions)
        return self._loaded(rc, lo[-1], None if k is None else ("list", k))

    def build(self, rows, nlist, keys=None, kmeans_iters=10, seed=20260320):
        rows = np.ascontiguousarray(rows, self.np_dtype)
        if rows.ndim != 2 or rows.shape[1] != self.row_words:
            return IndexError_.InvalidArgument
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_bivf_build(self._h, _np_ptr(rows), rows.shape[0], _np_ptr(k), int(nlist), int(kmeans_iters), int(seed))
        return self._loaded(rc, rows.shape[0], None if k is None else ("row", k))

    def build_dev(self, d_rows, n, nlist, keys=None, kmeans_iters=10, seed=20260320, stream=None):
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_bivf_build_dev(self._h, C.c_void_p(d_rows), int(n), _np_ptr(k), int(nlist), int(kmeans_iters), int(seed),
                                                C.c_void_p(stream) if stream else None)
        return self._loaded(rc, n, None if k is None else ("row", k))

    def info(self):
        n = C.c_uint64(0)
        nl = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_bivf_info(self._h, C.byref(n), C.byref(nl)), "zvec_hip_bivf_info")
        return int(n.value), int(nl.value)

    def export(self):
        """centroids [nlist][words], list_offsets [nlist + 1], row_ids [count] (original row of every list-order position)"""
        n, nlist = self.info()
        cent = np.zeros((nlist, self.row_words), self.np_dtype)
        lo = np.zeros(nlist + 1, np.uint64)
        rows = np.zeros(n, np.uint64)
        _lib.check(_lib.lib().zvec_hip_bivf_export(self._h, _np_ptr(cent), _np_ptr(lo), _np_ptr(rows)), "zvec_hip_bivf_export")
        return cent, lo, rows

    def get_vectors_by_ids(self, list_positions):
        pos = np.ascontiguousarray(list_positions, np.uint64)
        out = np.zeros((pos.size, self.row_words), self.np_dtype)
        _lib.check(_lib.lib().zvec_hip_bivf_get_vectors(self._h, _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_bivf_get_vectors")
        return out

    def keys_in_list_order(self):
        if self._list_keys is None:
            _, _, rows = self.export()
            if self._orig_keys is None:
                self._list_keys = rows
            else:
                kind, k = self._orig_keys
                self._list_keys = k if kind == "list" else k[rows.astype(np.int64)]
        return self._list_keys

    def _vectors_of_keys(self, keys):
        lk = self.keys_in_list_order()
        order = np.argsort(lk, kind="stable")
        return self.get_vectors_by_ids(order[np.searchsorted(lk[order], keys)])

    # IVFSearcherContext::update (ivf_searcher_context.h:61-79)
    def probe_params(self, ctx=None):
        ratio = self.scan_ratio if ctx is None or ctx._scan_ratio is None else ctx._scan_ratio
        bft = self.brute_force_threshold if ctx is None or ctx._bf_threshold is None else ctx._bf_threshold
        return ivf_probe_params(self.info()[1], self.total_count, ratio, bft)

    def set_nprobe(self, nprobe, exact=True):
        """as HipIVFSearcher.set_nprobe: scan_ratio = nprobe / nlist; exact=True keeps max_scan_count from cutting the probe loop"""
        self.scan_ratio = float(np.float32(nprobe) / np.float32(max(self.info()[1], 1)))
        if exact:
            self.brute_force_threshold = max(self.total_count - 1, 0)

    def search_impl(self, query, count, ctx, nprobe=None, max_scan=None):
        """IndexRunner::search_impl over the probed lists; nprobe / max_scan default to probe_params(ctx)"""
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(query, self.np_dtype).reshape(-1)
        if q.size != int(count) * self.row_words:
            return IndexError_.InvalidArgument
        k = ctx.topk()
        pp = self.probe_params(ctx) if nprobe is None or max_scan is None else (nprobe, max_scan)
        nprobe = pp[0] if nprobe is None else nprobe
        max_scan = pp[1] if max_scan is None else max_scan
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        if ctx._exclude is not None:
            ex = ctx._exclude
        else:
            ex = ctx._exclude_for(self.keys_in_list_order()) if ctx._filter_fn else None
        rc = _lib.lib().zvec_hip_bivf_search(self._h, ctx._h, _np_ptr(q), count, k, ctx.threshold(), int(nprobe), int(max_scan),
                                             _np_ptr(ex), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    def search_dev(self, d_queries, count, topk, nprobe, max_scan, d_out_keys, d_out_scores, d_out_counts, ctx, threshold=FLT_MAX,
                   d_exclude=None, stream=None):
        return _lib.lib().zvec_hip_bivf_search_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, threshold, nprobe, max_scan, C.c_void_p(d_exclude) if d_exclude else None,
            C.c_void_p(d_out_keys), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)

    def last_probes(self, ctx, count, nprobe):
        """(probe_idx [count][min(nprobe, nlist)], probe_cnt [count], scanned [count]) of the last search of this index on ctx,
        which was made with this nprobe"""
        idx = np.zeros((count, min(int(nprobe), self.info()[1])), np.uint32)
        cnt = np.zeros(count, np.uint32)
        scanned = np.zeros(count, np.uint32)
        _lib.check(_lib.lib().zvec_hip_bivf_last_probes(self._h, ctx._h, count, _np_ptr(idx), _np_ptr(cnt), _np_ptr(scanned)),
                   "zvec_hip_bivf_last_probes")
        return idx, cnt, scanned

    # ---- fed with fp32: rows kept in list order, candidates re-ranked on them (zvec_hip_bivf_*_fp32) ----
    def build_fp32(self, rows, nlist, metric="SquaredEuclidean", keys=None, kmeans_iters=10, seed=20260320, bin_threshold=0.0):
        """BinaryConverter + build + the fp32 rows gathered into list order; rows: [n][dim] fp32, self.dim == 32 * ceil(dim / 32)"""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2:
            return IndexError_.InvalidArgument
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_bivf_build_fp32(self._h, _np_ptr(rows), rows.shape[0], rows.shape[1], metric_from_name(metric), _np_ptr(k),
                                                 int(nlist), int(kmeans_iters), int(seed), float(bin_threshold))
        return self._loaded(rc, rows.shape[0], None if k is None else ("row", k))

    def build_fp32_dev(self, d_rows, n, dim, nlist, metric="SquaredEuclidean", keys=None, kmeans_iters=10, seed=20260320,
                       bin_threshold=0.0, stream=None):
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        rc = _lib.lib().zvec_hip_bivf_build_fp32_dev(self._h, C.c_void_p(d_rows), int(n), int(dim), metric_from_name(metric), _np_ptr(k),
                                                     int(nlist), int(kmeans_iters), int(seed), float(bin_threshold),
                                                     C.c_void_p(stream) if stream else None)
        return self._loaded(rc, n, None if k is None else ("row", k))

    def attach_rows(self, rows, metric="SquaredEuclidean"):
        """fp32 rows [count][dim], already in list order, for an index made by load or build; the bits are not checked against them"""
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[0] != self.info()[0]:
            return IndexError_.InvalidArgument
        return _lib.lib().zvec_hip_bivf_attach_rows(self._h, _np_ptr(rows), rows.shape[1], metric_from_name(metric))

    def attach_rows_dev(self, d_rows, dim, metric="SquaredEuclidean", stream=None):
        return _lib.lib().zvec_hip_bivf_attach_rows_dev(self._h, C.c_void_p(d_rows), int(dim), metric_from_name(metric),
                                                        C.c_void_p(stream) if stream else None)

    def rows_info(self):
        """(dim, metric, bytes) of the fp32 rows; dim 0: none"""
        d, m, b = C.c_uint32(0), C.c_int(0), C.c_uint64(0)
        _lib.check(_lib.lib().zvec_hip_bivf_rows_info(self._h, C.byref(d), C.byref(m), C.byref(b)), "zvec_hip_bivf_rows_info")
        return int(d.value), int(m.value), int(b.value)

    def get_rows_by_ids(self, list_positions):
        pos = np.ascontiguousarray(list_positions, np.uint64)
        out = np.zeros((pos.size, self.rows_info()[0]), np.float32)
        _lib.check(_lib.lib().zvec_hip_bivf_get_rows(self._h, _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_bivf_get_rows")
        return out

    def search_impl_fp32(self, queries, count, ctx, refine=4, bin_threshold=0.0, nprobe=None, max_scan=None):
        """fp32 queries ([count][dim]): BinaryReformer::transform, the Hamming search for min(topk * refine, 128) candidates and their
        re-rank on the fp32 rows, all on the GPU.  Results, filter and threshold (on the fp32 score) as search_impl."""
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim != 2 or q.shape[0] != int(count):
            return IndexError_.InvalidArgument
        k = ctx.topk()
        pp = self.probe_params(ctx) if nprobe is None or max_scan is None else (nprobe, max_scan)
        nprobe = pp[0] if nprobe is None else nprobe
        max_scan = pp[1] if max_scan is None else max_scan
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        if ctx._exclude is not None:
            ex = ctx._exclude
        else:
            ex = ctx._exclude_for(self.keys_in_list_order()) if ctx._filter_fn else None
        rc = _lib.lib().zvec_hip_bivf_search_fp32(self._h, ctx._h, _np_ptr(q), count, q.shape[1], k, int(refine), ctx.threshold(),
                                                  float(bin_threshold), int(nprobe), int(max_scan), _np_ptr(ex), _np_ptr(keys),
                                                  _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts, self._vectors_of_keys)
        return rc

    def search_fp32_dev(self, d_queries, dim, count, topk, refine, nprobe, max_scan, d_out_keys, d_out_scores, d_out_counts, ctx,
                        bin_threshold=0.0, threshold=FLT_MAX, d_exclude=None, stream=None):
        """device-pointer form of search_impl_fp32 (async): all arguments are raw device pointers (ints)."""
        return _lib.lib().zvec_hip_bivf_search_fp32_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, int(dim), topk, int(refine), threshold, float(bin_threshold), nprobe, max_scan,
            C.c_void_p(d_exclude) if d_exclude else None, C.c_void_p(d_out_keys), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts),
            C.c_void_p(stream) if stream else None)

    def last_candidates(self, ctx, count, kc):
        """(positions [count][kc], hamming_scores [count][kc], counts [count]): stage 1 of the last fp32 search of this index on ctx,
        which ran with kc = min(topk * refine, 128)"""
        pos = np.zeros((count, kc), np.uint32)
        sc = np.zeros((count, kc), np.float32)
        cnt = np.zeros(count, np.uint32)
        _lib.check(_lib.lib().zvec_hip_bivf_last_candidates(self._h, ctx._h, count, kc, _np_ptr(pos), _np_ptr(sc), _np_ptr(cnt)),
                   "zvec_hip_bivf_last_candidates")
        return pos, sc, cnt


class HipHnswSearcher:
    """Batched k-NN search on a built HNSW graph (zvec_hip_hnsw_*): what HnswSearcher::search_impl is above its brute-force
    hand-over.  fp32 or fp16 rows, "SquaredEuclidean" or "InnerProduct".  The graph is loaded as plain arrays, or built from rows
    (build).  dtype="fp16" (zvec_hip_hnsw_create_typed): rows and queries are stored and passed as IEEE binary16; load / build / add /
    search take float16 arrays as they are and round float32 arrays to nearest even (astype(float16), what HalfFloatConverter does);
    the _dev variants take raw pointers to halves; get_vectors_by_ids returns float16.  Scores are fp32."""

    def __init__(self, dim, metric="SquaredEuclidean", device=0, dtype="fp32"):
        self.dim = int(dim)
        self.metric = metric_from_name(metric) if isinstance(metric, str) else int(metric)
        self.device = device
        self.dtype, self.np_dtype = _dtype_of(dtype)
        self._h = C.c_void_p()
        create = "zvec_hip_hnsw_create_typed" if self.dtype == DT_FP16 else "zvec_hip_hnsw_create"
        _lib.check(getattr(_lib.lib(), create)(self.dim, self.dtype, self.metric, device, C.byref(self._h)), create)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_hnsw_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def create_context(self):
        return IndexContext(self.device)

    def load(self, rows, nbr0, cnt0, entry_point=0, keys=None, upper_of=None, nbr_up=None, cnt_up=None):
        """rows [n][dim]; nbr0 [n][m0] with cnt0 [n]; upper levels (all three or none): upper_of [n], nbr_up [n_upper][max_level][m],
        cnt_up [n_upper][max_level]"""
        rows = np.ascontiguousarray(rows, self.np_dtype)
        n = rows.shape[0]
        if rows.ndim != 2 or (n and rows.shape[1] != self.dim):
            return IndexError_.Mismatch
        nbr0 = np.ascontiguousarray(nbr0, np.uint32).reshape(n, -1) if n else np.zeros((0, 1), np.uint32)
        cnt0 = np.ascontiguousarray(cnt0, np.uint32)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        if cnt0.size != n or (k is not None and k.size != n):
            return IndexError_.InvalidArgument
        max_level = m = n_upper = 0
        if nbr_up is not None and n:
            upper_of = np.ascontiguousarray(upper_of, np.uint32)
            nbr_up = np.ascontiguousarray(nbr_up, np.uint32)
            cnt_up = np.ascontiguousarray(cnt_up, np.uint32)
            if nbr_up.ndim != 3 or cnt_up.shape != nbr_up.shape[:2] or upper_of.size != n:
                return IndexError_.InvalidArgument
            n_upper, max_level, m = nbr_up.shape
        if max_level == 0:
            upper_of = nbr_up = cnt_up = None
        return _lib.lib().zvec_hip_hnsw_load(self._h, n, _np_ptr(rows), _np_ptr(k), nbr0.shape[1], _np_ptr(nbr0), _np_ptr(cnt0), max_level, m,
                                             n_upper, _np_ptr(upper_of), _np_ptr(nbr_up), _np_ptr(cnt_up), int(entry_point))

    def _build_args(self, n, keys, levels, m, m0, ef_construction, prune_cnt, min_neighbors, scaling_factor, seed):
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        lv = None if levels is None else np.ascontiguousarray(levels, np.uint32)
        if (k is not None and k.size != n) or (lv is not None and lv.size != n):
            return None
        p = _lib.HnswBuildParams(int(m), int(m0), int(ef_construction), int(prune_cnt), int(min_neighbors), int(scaling_factor),
                                 int(seed) & 0xffffffffffffffff)
        return k, lv, p

    def build(self, rows, keys=None, levels=None, m=0, m0=0, ef_construction=0, prune_cnt=0, min_neighbors=0, scaling_factor=0, seed=0):
        """HnswBuilder::build: rows [n][dim] in, searchable graph out, by the rounds of DESIGN §3c.  An argument left 0 takes the
        reference's default (m 50, m0 2m, ef_construction 500, prune_cnt m, scaling_factor m); levels [n] or None = generated
        (hnsw_levels).  Returns 0 or a negative IndexError value."""
        rows = np.ascontiguousarray(rows, self.np_dtype)
        n = rows.shape[0]
        if rows.ndim != 2 or (n and rows.shape[1] != self.dim):
            return IndexError_.Mismatch
        args = self._build_args(n, keys, levels, m, m0, ef_construction, prune_cnt, min_neighbors, scaling_factor, seed)
        if args is None:
            return IndexError_.InvalidArgument
        k, lv, p = args
        return _lib.lib().zvec_hip_hnsw_build(self._h, n, _np_ptr(rows), _np_ptr(k), C.byref(p), _np_ptr(lv))

    def build_dev(self, d_rows, n, keys=None, levels=None, m=0, m0=0, ef_construction=0, prune_cnt=0, min_neighbors=0, scaling_factor=0,
                  seed=0):
        """build with rows [n][dim] of the searcher's dtype in device memory (a raw device pointer); keys and levels stay host arrays"""
        args = self._build_args(int(n), keys, levels, m, m0, ef_construction, prune_cnt, min_neighbors, scaling_factor, seed)
        if args is None:
            return IndexError_.InvalidArgument
        k, lv, p = args
        return _lib.lib().zvec_hip_hnsw_build_dev(self._h, int(n), C.c_void_p(d_rows), _np_ptr(k), C.byref(p), _np_ptr(lv))

    def build_info(self):
        """{rounds, slices, top, entry_point, dists, requests, prunes, insert_ms, reverse_ms} of the last build"""
        out = _lib.HnswBuildInfo()
        _lib.check(_lib.lib().zvec_hip_hnsw_last_build_info(self._h, C.byref(out)), "zvec_hip_hnsw_last_build_info")
        return {k: getattr(out, k) for k, _ in out._fields_}

    def _add_args(self, n, keys, levels, params):
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        lv = None if levels is None else np.ascontiguousarray(levels, np.uint32)
        if (k is not None and k.size != n) or (lv is not None and lv.size != n):
            return None
        names = [f for f, _ in _lib.HnswBuildParams._fields_]
        if any(x not in names for x in params):
            raise TypeError("unknown HNSW parameter among %s" % sorted(params))
        p = None
        if params:
            p = _lib.HnswBuildParams(*[int(params.get(f, 0)) & (0xffffffffffffffff if f == "seed" else 0xffffffff) for f in names])
        return k, lv, p

    def add(self, rows, keys=None, levels=None, **params):
        """HnswStreamer::add_impl for rows [count][dim] at once: they take the positions n .. n + count - 1 and are inserted by the
        rounds of DESIGN §3c "Appending".  params (m, m0, ef_construction, prune_cnt, min_neighbors, scaling_factor, seed): one left
        out or 0 takes the value of the last build (the reference's default on a loaded handle).  Returns 0 or a negative
        IndexError value."""
        rows = np.ascontiguousarray(rows, self.np_dtype)
        n = rows.shape[0]
        if rows.ndim != 2 or (n and rows.shape[1] != self.dim):
            return IndexError_.Mismatch
        args = self._add_args(n, keys, levels, params)
        if args is None:
            return IndexError_.InvalidArgument
        k, lv, p = args
        return _lib.lib().zvec_hip_hnsw_add(self._h, n, _np_ptr(rows), _np_ptr(k), C.byref(p) if p is not None else None, _np_ptr(lv))

    def add_dev(self, d_rows, n, keys=None, levels=None, **params):
        """add with rows [n][dim] of the searcher's dtype in device memory (a raw device pointer); keys and levels stay host arrays"""
        args = self._add_args(int(n), keys, levels, params)
        if args is None:
            return IndexError_.InvalidArgument
        k, lv, p = args
        return _lib.lib().zvec_hip_hnsw_add_dev(self._h, int(n), C.c_void_p(d_rows), _np_ptr(k), C.byref(p) if p is not None else None,
                                                _np_ptr(lv))

    def reserve(self, rows, upper_nodes=0):
        """room for `rows` rows and `upper_nodes` nodes of level >= 1 (0: chosen from the scaling factor), so that adds up to there
        move nothing; never shrinks"""
        return _lib.lib().zvec_hip_hnsw_reserve(self._h, int(rows), int(upper_nodes))

    def add_info(self):
        """the fields of build_info for the last add alone, and {first, count, rounds_one, grew_rows, grew_upper, restrided,
        cap_rows, cap_upper}"""
        out = _lib.HnswAddInfo()
        _lib.check(_lib.lib().zvec_hip_hnsw_last_add_info(self._h, C.byref(out)), "zvec_hip_hnsw_last_add_info")
        return {k: getattr(out, k) for k, _ in out._fields_}

    def info(self):
        """{n, dim, m0, max_level, m, n_upper, entry_point}"""
        n = C.c_uint64(0)
        v = [C.c_uint32(0) for _ in range(6)]
        _lib.check(_lib.lib().zvec_hip_hnsw_info(self._h, C.byref(n), *[C.byref(x) for x in v]), "zvec_hip_hnsw_info")
        names = ("dim", "m0", "max_level", "m", "n_upper", "entry_point")
        return dict([("n", int(n.value))] + [(k, int(x.value)) for k, x in zip(names, v)])

    def get_vectors_by_ids(self, positions):
        pos = np.ascontiguousarray(positions, np.uint64)
        out = np.zeros((pos.size, self.dim), self.np_dtype)
        _lib.check(_lib.lib().zvec_hip_hnsw_get_vectors(self._h, _np_ptr(pos), pos.size, _np_ptr(out)), "zvec_hip_hnsw_get_vectors")
        return out

    def export(self):
        """keys, nbr0, cnt0, upper_of, nbr_up, cnt_up as load took them (the upper three None without upper levels)"""
        i = self.info()
        n = i["n"]
        keys, nbr0, cnt0 = np.zeros(n, np.uint64), np.zeros((n, i["m0"]), np.uint32), np.zeros(n, np.uint32)
        up = i["max_level"] > 0
        upper_of = np.zeros(n, np.uint32) if up else None
        nbr_up = np.zeros((i["n_upper"], i["max_level"], i["m"]), np.uint32) if up else None
        cnt_up = np.zeros((i["n_upper"], i["max_level"]), np.uint32) if up else None
        _lib.check(_lib.lib().zvec_hip_hnsw_export(self._h, _np_ptr(keys), _np_ptr(nbr0), _np_ptr(cnt0), _np_ptr(upper_of), _np_ptr(nbr_up),
                                                   _np_ptr(cnt_up)), "zvec_hip_hnsw_export")
        return keys, nbr0, cnt0, upper_of, nbr_up, cnt_up

    def search(self, query, count, ctx, ef, max_scan=0):
        """HnswSearcher::search_impl: topk, threshold and the exclude bitset (1 bit per node) come from ctx; ef and max_scan are
        HnswContext's.  Fills ctx like search_impl of the other searchers and returns 0 or a negative IndexError value."""
        if ctx is None or ctx.topk() == 0:
            return IndexError_.InvalidArgument
        q = np.ascontiguousarray(query, self.np_dtype).reshape(int(count), -1)
        if q.shape[1] != self.dim:
            return IndexError_.Mismatch
        k = ctx.topk()
        keys = np.zeros((count, k), np.uint64)
        scores = np.zeros((count, k), np.float32)
        counts = np.zeros(count, np.uint32)
        rc = _lib.lib().zvec_hip_hnsw_search(self._h, ctx._h, _np_ptr(q), count, k, int(ef), int(max_scan), ctx.threshold(),
                                             _np_ptr(ctx._exclude), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        if rc == 0:
            ctx._set_results(keys, scores, counts)
        return rc

    def search_dev(self, d_queries, count, topk, ef, max_scan, d_out_keys, d_out_scores, d_out_counts, ctx, threshold=FLT_MAX,
                   d_exclude=None, stream=None):
        """device-pointer form (async): all arguments are raw device pointers (ints); the queries are of the searcher's dtype"""
        return _lib.lib().zvec_hip_hnsw_search_dev(
            self._h, ctx._h, C.c_void_p(d_queries), count, topk, int(ef), int(max_scan), threshold, C.c_void_p(d_exclude) if d_exclude else None,
            C.c_void_p(d_out_keys), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream) if stream else None)

    def last_stats(self, ctx, count):
        """(distances computed [count], nodes expanded on level 0 [count], slices) of the last search of this index on ctx"""
        scanned = np.zeros(count, np.uint32)
        hops = np.zeros(count, np.uint32)
        slices = C.c_uint32(0)
        _lib.check(_lib.lib().zvec_hip_hnsw_last_stats(self._h, ctx._h, count, _np_ptr(scanned), _np_ptr(hops), C.byref(slices)),
                   "zvec_hip_hnsw_last_stats")
        return scanned, hops, int(slices.value)


def hnsw_levels(n, scaling_factor, seed=0):
    """the levels zvec_hip_hnsw_build gives n nodes when it is passed none (zvec_hip_hnsw_build_levels; host only)"""
    out = np.zeros(int(n), np.uint32)
    _lib.check(_lib.lib().zvec_hip_hnsw_build_levels(int(n), int(scaling_factor), int(seed) & 0xffffffffffffffff, _np_ptr(out)),
               "zvec_hip_hnsw_build_levels")
    return out


def container_segments(image, checksum=False):
    """segment table of a dumped index FILE image (zvec_hip_container_segments): {id: (offset, size)} in file order"""
    image = bytes(image)
    n = C.c_uint32(0)
    L = _lib.lib()
    _lib.check(L.zvec_hip_container_segments(image, len(image), int(checksum), None, 0, C.byref(n)), "zvec_hip_container_segments")
    arr = (_lib.Segment * max(int(n.value), 1))()
    _lib.check(L.zvec_hip_container_segments(image, len(image), int(checksum), arr, n.value, C.byref(n)), "zvec_hip_container_segments")
    return {arr[i].id.decode(): (int(arr[i].offset), int(arr[i].size)) for i in range(n.value)}


def parse_index_meta(blob):
    """the "IndexMeta" segment: IndexMetaFormatHeader (src/core/framework/index_meta.cc:23-34) + its JSON attachment
    (metric name under "metric"."name", index_meta.cc:39-80)"""
    import json
    import struct
    hs, meta_type, major, dt, dim, unit, space, aoff, asz = struct.unpack_from("<9I", blob, 0)
    metric, att = None, {}
    if asz:                               # attachment_offset counts from the start of the blob (index_meta.cc:62-80)
        try:
            att = json.loads(bytes(blob[aoff:aoff + asz]).decode())
            metric = att.get("metric", {}).get("name")
        except (ValueError, UnicodeDecodeError):
            metric, att = None, {}
    out = {"major_order": major, "data_type": dt, "dimension": dim, "unit_size": unit, "metric": metric}
    for role in ("builder", "searcher", "streamer"):      # index_meta.cc:80-107
        out[role + "_name"] = att.get(role, {}).get("name")
        out[role + "_params"] = att.get(role, {}).get("params", {})
    return out


def open_flat_file(image, device=0, metric=None):
    """FlatSearcher::load from a dumped flat index FILE (container -> "IndexMeta" / "flat.keys" / "flat.features")"""
    image = bytes(image)
    seg = container_segments(image)
    meta = parse_index_meta(image[seg["IndexMeta"][0]:sum(seg["IndexMeta"])])
    dtype = "fp16" if meta["data_type"] == 1 else "fp32"
    se = HipFlatSearcher(meta["dimension"], metric or meta["metric"] or "SquaredEuclidean", device=device, dtype=dtype)
    ko, ks = seg["flat.keys"]
    fo, fs_ = seg["flat.features"]
    keys = np.frombuffer(image, np.uint64, ks // 8, ko)
    _lib.check(se.load_features(image[fo:fo + fs_], ks // 8, column_major=(meta["major_order"] == 2), keys=keys), "load_features")
    return se


def open_ivf_file(image, device=0, metric=None):
    """IVFSearcher::load from a dumped IVF index FILE: the ivf.* / hc.keys segments, and the centroid rows out of the
    NESTED flat index file that the "ivf.centroid" segment holds (ivf_searcher.cc:43-103)"""
    image = bytes(image)
    seg = container_segments(image)
    meta = parse_index_meta(image[seg["IndexMeta"][0]:sum(seg["IndexMeta"])])
    dtype = "fp16" if meta["data_type"] == 1 else "fp32"
    npdt = np.float16 if dtype == "fp16" else np.float32
    co, cs = seg["ivf.centroid"]
    nested = image[co:co + cs]
    cseg = container_segments(nested)
    cmeta = parse_index_meta(nested[cseg["IndexMeta"][0]:sum(cseg["IndexMeta"])])
    ck = np.frombuffer(nested, np.uint64, cseg["flat.keys"][1] // 8, cseg["flat.keys"][0])
    nlist, dim = ck.size, meta["dimension"]
    feat = np.frombuffer(nested, npdt, nlist * dim, cseg["flat.features"][0]).copy()
    rows = np.empty((nlist, dim), npdt)
    if cmeta["major_order"] == 2:                       # column-major centroid index: full 32-row blocks are transposed
        full = nlist // 32 * 32
        rows[:full] = feat[:full * dim].reshape(full // 32, dim, 32).transpose(0, 2, 1).reshape(full, dim)
        rows[full:] = feat[full * dim:].reshape(nlist - full, dim)
    else:
        rows[:] = feat.reshape(nlist, dim)
    cent = np.empty_like(rows)
    cent[ck.astype(np.int64)] = rows                    # row i of the centroid index holds centroid ck[i]
    se = HipIVFSearcher(dim, metric or meta["metric"] or "SquaredEuclidean", device=device, dtype=dtype)

    def payload(name):
        o, sz = seg[name]
        return image[o:o + sz]
    _lib.check(se.load_segments(payload("ivf.inverted_header"), payload("ivf.inverted_meta"), payload("ivf.inverted_body"),
                                payload("hc.keys"), cent), "load_segments")
    return se


class Gate:
    """zvec_hip_gate_t: contexts sharing it take turns on their dominant scan kernel (pipelining consecutive batches)"""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_gate_create(int(device), C.byref(self._h)), "zvec_hip_gate_create")

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_gate_destroy(self._h)
                self._h = None
        except Exception:
            pass


class HipShardedIndex:
    """one index over several GPUs inside ONE process (zvec_hip_shards_*): the in-process counterpart of the
    one-rank-per-GPU sharding in zvec_amd/dist.py, for embedded callers like zvec itself.  kind: "flat" or "ivf";
    devices: HIP device ordinals, repeats allowed (several shards on one GPU)."""

    def __init__(self, kind, dim, metric=METRIC_L2, devices=(0,), dtype="fp32"):
        if isinstance(metric, str):
            metric = metric_from_name(metric)
        self.kind = {"flat": 0, "ivf": 1}[kind]
        self.dim = int(dim)
        self.dtype, self.np_dtype = _dtype_of(dtype)
        self.ndev = len(devices)
        dev = (C.c_int * self.ndev)(*[int(d) for d in devices])
        self._h = C.c_void_p()
        _lib.check(_lib.lib().zvec_hip_shards_create(self.dim, self.dtype, metric, self.kind, dev, self.ndev, C.byref(self._h)),
                   "zvec_hip_shards_create")

    def __del__(self):
        try:
            if self._h:
                _lib.lib().zvec_hip_shards_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def counts(self):
        total = C.c_uint64(0)
        per = np.zeros(self.ndev, np.uint64)
        _lib.check(_lib.lib().zvec_hip_shards_count(self._h, C.byref(total), _np_ptr(per)), "zvec_hip_shards_count")
        return int(total.value), per

    def append(self, vecs, keys=None):
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        return _lib.lib().zvec_hip_shards_flat_append(self._h, _np_ptr(vecs), vecs.shape[0], _np_ptr(k))

    def build(self, vecs, nlist, keys=None, kmeans_iters=10, sample_per_list=256, seed=20260320):
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        return _lib.lib().zvec_hip_shards_ivf_build(self._h, _np_ptr(vecs), vecs.shape[0], _np_ptr(k), nlist, kmeans_iters,
                                                    sample_per_list, seed)

    def load(self, centroids, list_offsets, vecs, keys=None):
        centroids = np.ascontiguousarray(centroids, self.np_dtype)
        lo = np.ascontiguousarray(list_offsets, np.uint64)
        vecs = np.ascontiguousarray(vecs, self.np_dtype)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        return _lib.lib().zvec_hip_shards_ivf_load(self._h, _np_ptr(centroids), centroids.shape[0], _np_ptr(lo), _np_ptr(vecs),
                                                   _np_ptr(k))

    def load_segments(self, inverted_header, inverted_meta, inverted_body, keys, centroids):
        cent = np.ascontiguousarray(centroids, self.np_dtype)
        hb, mb, bb, kb = bytes(inverted_header), bytes(inverted_meta), bytes(inverted_body), bytes(keys)
        return _lib.lib().zvec_hip_shards_ivf_load_segments(self._h, hb, len(hb), mb, len(mb), bb, len(bb), kb, len(kb), _np_ptr(cent))

    def load_features(self, features, count, column_major=False, batch_size=32, keys=None):
        fb = bytes(features)
        k = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        return _lib.lib().zvec_hip_shards_flat_load_features(self._h, fb, len(fb), int(count), int(bool(column_major)),
                                                             int(batch_size), _np_ptr(k))

    def search_by_ids(self, queries, ids_per_query, topk, threshold=FLT_MAX, exclude=None):
        """search_bf_by_p_keys_impl over the shards: ids are global storage positions."""
        q = np.ascontiguousarray(queries, self.np_dtype)
        count = q.shape[0]
        offs = np.zeros(count + 1, np.uint32)
        offs[1:] = np.cumsum([len(x) for x in ids_per_query])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint64) for x in ids_per_query] + [np.zeros(1, np.uint64)]))
        ex = None if exclude is None else np.ascontiguousarray(exclude, np.uint64)
        keys = np.empty((count, topk), np.uint64)
        scores = np.empty((count, topk), np.float32)
        counts = np.empty(count, np.uint32)
        _lib.check(_lib.lib().zvec_hip_shards_flat_search_by_ids(self._h, _np_ptr(q), count, _np_ptr(ids), _np_ptr(offs), int(topk),
                                                                 float(threshold), _np_ptr(ex), _np_ptr(keys), _np_ptr(scores),
                                                                 _np_ptr(counts)), "zvec_hip_shards_flat_search_by_ids")
        return keys, scores, counts

    def get_vectors(self, positions):
        pos = np.ascontiguousarray(positions, np.uint64)
        out = np.empty((pos.size, self.dim), self.np_dtype)
        rc = _lib.lib().zvec_hip_shards_flat_get_vectors(self._h, _np_ptr(pos), pos.size, _np_ptr(out))
        return rc, out

    def deal_coarse(self, enable):
        """IVF: deal the coarse pass over the shards (zvec_hip_shards_deal_coarse; off by default)"""
        return _lib.lib().zvec_hip_shards_deal_coarse(self._h, int(bool(enable)))

    def search(self, queries, topk, nprobe=1, max_scan=0xffffffff, threshold=FLT_MAX, exclude=None):
        q = np.ascontiguousarray(queries, self.np_dtype)
        count = q.shape[0]
        keys = np.zeros((count, topk), np.uint64)
        scores = np.zeros((count, topk), np.float32)
        counts = np.zeros(count, np.uint32)
        ex = None if exclude is None else np.ascontiguousarray(exclude, np.uint64)
        rc = _lib.lib().zvec_hip_shards_search(self._h, _np_ptr(q), count, topk, threshold, nprobe, max_scan, _np_ptr(ex),
                                               _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
        _lib.check(rc, "zvec_hip_shards_search")
        return keys, scores, counts


def normalize_score(metric, score):
    """what core_interface::Index::_dense_search applies ABOVE boundary B (index.cc:624-630): metric->normalize() —
    InnerProductMetric::normalize negates the kernel's minus-inner-product back to +ip (inner_product_metric.cc:377-384);
    SquaredEuclidean and Cosine ("1 - ip" already) have no normalize step."""
    if isinstance(metric, str):
        metric = metric_from_name(metric)
    return -score if metric == METRIC_IP else score


def ivf_probe_params(nlist, n, scan_ratio, brute_force_threshold):
    """IVFSearcherContext::update (ivf_searcher_context.h:61-79) in the reference's float arithmetic:
    nprobe = max(round(nlist * scan_ratio), 1) (std::round: half away from zero),
    max_scan_count = max(brute_force_threshold, ceil(N * scan_ratio))."""
    nprobe = max(int(np.floor(np.float32(np.float32(nlist) * np.float32(scan_ratio)) + np.float32(0.5))), 1)
    max_scan = int(np.ceil(np.float32(np.float32(n) * np.float32(scan_ratio))))
    return nprobe, max(int(brute_force_threshold), max_scan)


def shard_map(list_sizes, nshards):
    """list -> shard map of zvec_hip_ivf_shard_map (pure host arithmetic): (owner[nlist], rows per shard)."""
    sz = np.ascontiguousarray(list_sizes, np.uint32)
    owner = np.zeros(sz.size, np.uint32)
    rows = np.zeros(nshards, np.uint64)
    _lib.check(_lib.lib().zvec_hip_ivf_shard_map(_np_ptr(sz), sz.size, int(nshards), _np_ptr(owner), _np_ptr(rows)),
               "zvec_hip_ivf_shard_map")
    return owner, rows


def merge_topk(ctx, keys, scores, counts, topk):
    """host form of the shard merge: inputs [nparts][count][topk] / [nparts][count]."""
    keys = np.ascontiguousarray(keys, np.uint64)
    scores = np.ascontiguousarray(scores, np.float32)
    counts = np.ascontiguousarray(counts, np.uint32)
    nparts, count = counts.shape
    ok = np.zeros((count, topk), np.uint64)
    os_ = np.zeros((count, topk), np.float32)
    oc = np.zeros(count, np.uint32)
    _lib.check(_lib.lib().zvec_hip_merge_topk(ctx._h, _np_ptr(keys), _np_ptr(scores), _np_ptr(counts), nparts,
                                              count, topk, _np_ptr(ok), _np_ptr(os_), _np_ptr(oc)),
               "zvec_hip_merge_topk")
    return ok, os_, oc
