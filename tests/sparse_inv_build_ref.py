"""Numpy models of the term-major twin of a sparse index and of the device build's radix sort (zvk_sparse_invb.hip.h), and the
cases tests/test_sparse_inv_build_reference_cpu.py and tests/test_gpu_sparse_inverted_build.py share.

twin_model     what the twin must hold: a stable argsort of the stored elements by index; heads, offsets and positions by
               np.repeat; values gathered as raw bytes.
radix_model    the same arrays by the scheme the device uses: digit passes chosen from the OR of the indices, per-block digit
               histograms in a [digit][block] table, one exclusive scan over the table, a scatter that keeps equal digits in
               element order.  The block size is a parameter.

A case is (counts, indices, values): CSR-like rows, indices strictly ascending inside a row."""
import numpy as np

W = 64      # lanes of a wave


def np_dtype(dtype):
    return np.float16 if dtype == "fp16" else np.float32


def raw(values):
    """the values as unsigned words of their own width: compared bit for bit (-0.0 != 0.0 here, and a NaN equals itself)"""
    v = np.ascontiguousarray(values)
    return v.view(np.uint16 if v.dtype.itemsize == 2 else np.uint32)


def passes_of(indices):
    """8-bit digit passes the sort needs: ceil(bits(OR of the indices) / 8), 0 when every index is 0 (or there is none)"""
    o = int(np.bitwise_or.reduce(np.asarray(indices, np.uint32))) if len(indices) else 0
    return (o.bit_length() + 7) // 8


def _finish(counts, indices, values, order):
    """terms, list_off, ppos, pval (raw words) from the sorted order of the elements"""
    counts = np.asarray(counts, np.int64)
    indices = np.asarray(indices, np.uint32)
    pos = np.repeat(np.arange(counts.size, dtype=np.uint32), counts)
    sidx = indices[order]
    head = np.ones(sidx.size, bool)
    head[1:] = sidx[1:] != sidx[:-1]
    starts = np.nonzero(head)[0]
    list_off = np.concatenate([starts, [sidx.size]]).astype(np.uint64)
    return sidx[starts].astype(np.uint32), list_off, pos[order], raw(values)[order]


def twin_model(counts, indices, values):
    order = np.argsort(np.asarray(indices, np.uint32), kind="stable")
    return _finish(counts, indices, values, order)


def radix_sort_order(indices, block):
    """(order, passes): the element ordinals after the stable least-significant-digit sort, 8 bits per pass, `block` elements per
    work-group; every pass is histogram table -> exclusive scan -> scatter"""
    keys = np.asarray(indices, np.uint32).copy()
    E = keys.size
    order = np.arange(E, dtype=np.uint32)
    passes = passes_of(keys)
    nblocks = (E + block - 1) // block
    for p in range(passes):
        digit = ((keys >> np.uint32(8 * p)) & np.uint32(255)).astype(np.int64)
        blk = np.arange(E, dtype=np.int64) // block
        table = np.zeros((256, nblocks), np.int64)
        np.add.at(table, (digit, blk), 1)
        flat = table.reshape(-1)
        scanned = (np.cumsum(flat) - flat).reshape(256, nblocks)
        dst = np.empty(E, np.int64)
        for b in range(nblocks):
            lo, hi = b * block, min(E, (b + 1) * block)
            d = digit[lo:hi]
            # rank of an element among the block's elements of the same digit, in element order
            rank = np.empty(hi - lo, np.int64)
            seen = np.zeros(256, np.int64)
            for j, dj in enumerate(d):
                rank[j] = seen[dj]
                seen[dj] += 1
            dst[lo:hi] = scanned[d, b] + rank
        assert np.array_equal(np.sort(dst), np.arange(E))
        nk, no = np.empty_like(keys), np.empty_like(order)
        nk[dst], no[dst] = keys, order
        keys, order = nk, no
    return order, passes


def radix_model(counts, indices, values, block):
    order, passes = radix_sort_order(indices, block)
    return _finish(counts, indices, values, order), passes


def same_twin(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def special_values(rng, size, dtype):
    """finite values of the handle's type with -0.0, denormals and (fp16) the smallest and largest patterns sprinkled in"""
    t = np_dtype(dtype)
    v = rng.standard_normal(size).astype(t)
    if dtype == "fp16":
        pool = np.array([0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff, 0xfbff, 0x0000], np.uint16).view(np.float16)
    else:
        pool = np.array([0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x00000000], np.uint32).view(np.float32)
    at = rng.random(size) < 0.25
    v[at] = pool[rng.integers(0, pool.size, int(at.sum()))]
    return v


def counts_for(rng, elems, lo=1, hi=5):
    """row lengths in [lo, hi] that add up to exactly `elems`"""
    out, left = [], int(elems)
    while left > 0:
        c = min(left, int(rng.integers(lo, hi + 1)))
        out.append(c)
        left -= c
    return np.asarray(out, np.uint32)


def rows_from(rng, counts, vocab, dtype, pick=None):
    """rows of the given lengths over indices drawn from `vocab` (an int: range(vocab); an array: its entries), ascending in a row"""
    pool = np.arange(vocab, dtype=np.uint32) if np.isscalar(vocab) else np.asarray(vocab, np.uint32)
    runs = [np.sort(rng.choice(pool, int(c), replace=False)) for c in counts]
    indices = np.concatenate(runs).astype(np.uint32) if runs else np.zeros(0, np.uint32)
    return np.asarray(counts, np.uint32), indices, special_values(rng, indices.size, dtype)


def edge_sizes(B):
    return [1, W - 1, W, W + 1, B - 1, B, B + 1, 3 * B + 17]


def edge_case(E, dtype, seed=0):
    """E elements in rows of 1 to 5, indices below 1000 (two digit passes)"""
    rng = np.random.default_rng(1000 + seed + E)
    return rows_from(rng, counts_for(rng, E), 1000, dtype)


def single_list_case(B, dtype):
    """one index shared by every row: a single list of E = 2B + 5 postings"""
    rng = np.random.default_rng(21)
    n = 2 * B + 5
    return np.ones(n, np.uint32), np.full(n, 77, np.uint32), special_values(rng, n, dtype)


def alternating_case(B, dtype):
    """two indices with the same low byte and different second bytes, alternating row by row"""
    rng = np.random.default_rng(22)
    n = 2 * B + 5
    indices = np.where(np.arange(n) % 2 == 0, 0x0305, 0x0105).astype(np.uint32)
    return np.ones(n, np.uint32), indices, special_values(rng, n, dtype)


PASS_CASES = [("zero", [0], 0), ("255", [3, 255], 1), ("256", [7, 256], 2), ("65535", [7, 300, 65535], 2), ("65536", [9, 65536], 3),
              ("max", [0, 0xffffffff], 4)]


def pass_case(name, dtype, elems=700):
    """rows of one element each over a small set of indices whose maximum pins the pass count"""
    pool, want = next((p, w) for n, p, w in PASS_CASES if n == name)
    rng = np.random.default_rng(23)
    indices = np.asarray(pool, np.uint32)[rng.integers(0, len(pool), elems)]
    indices[:len(pool)] = pool                                          # every index of the set is there
    return (np.ones(elems, np.uint32), indices, special_values(rng, elems, dtype)), want


def zero_low_digit_case(dtype, elems=3000):
    """every index a multiple of 256 below 65 536: the low digit is zero everywhere, the OR still asks for two passes"""
    rng = np.random.default_rng(24)
    return rows_from(rng, counts_for(rng, elems), np.arange(256, 65536, 256), dtype)


def ragged_case(B, dtype):
    """empty rows interleaved, one row of 300 elements placed so that it spans a block boundary when B allows, the last row empty"""
    rng = np.random.default_rng(25)
    lead = counts_for(rng, max(B - 150, 1))                             # the long row starts 150 elements before the boundary
    counts = []
    for c in lead:
        counts += [int(c), 0]
    counts += [300, 0, 0] + [int(c) for c in counts_for(rng, B + 40)] + [0]
    return rows_from(rng, np.asarray(counts, np.uint32), 5000, dtype)


def empty_rows_case(dtype):
    """rows, but no element"""
    return np.zeros(5, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np_dtype(dtype))


def no_rows_case(dtype):
    return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np_dtype(dtype))


def zipf_case(n, vocab, dtype, seed=26):
    """a corpus of n rows of 1 to 20 elements over a Zipf vocabulary; it is searched, so the values are small non-zero integers,
    |v| <= 8: products and sums of up to 20 of them are exact in fp32 (and every value in fp16) in any order of summation"""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, vocab + 1)
    w /= w.sum()
    counts = rng.integers(1, 21, n).astype(np.uint32)
    runs = [np.sort(rng.choice(vocab, int(c), replace=False, p=w)) for c in counts]
    indices = np.concatenate(runs).astype(np.uint32)
    values = (rng.integers(1, 9, indices.size) * rng.choice([-1, 1], indices.size)).astype(np_dtype(dtype))
    return counts, indices, values


def all_cases(B, dtype):
    """name -> case, for every case the GPU file builds (the CPU file runs both models over all of them)"""
    out = {"edge_%d" % E: edge_case(E, dtype) for E in edge_sizes(B)}
    out["single_list"] = single_list_case(B, dtype)
    out["alternating"] = alternating_case(B, dtype)
    for name, _, _ in PASS_CASES:
        out["pass_" + name] = pass_case(name, dtype)[0]
    out["zero_low_digit"] = zero_low_digit_case(dtype)
    out["ragged"] = ragged_case(B, dtype)
    out["empty_rows"] = empty_rows_case(dtype)
    out["no_rows"] = no_rows_case(dtype)
    return out
