"""Model of the Hamming IVF index fed with fp32 (numpy only; nothing here touches the GPU or the library): the fp64 scores of the
re-rank, the error band of an fp32 score, the checker of stage 1 (the Hamming candidates read back), the checker of stage 2 given
those candidates, and the fixtures of tests/test_gpu_hamming_ivf_fp32.py.  tests/test_hamming_ivf_fp32_reference_cpu.py holds the
fixtures to their preconditions and the checkers to hand-made wrong answers.

Band.  An fp32 sum of `dim` terms accumulated with fma in any order is within gamma_dim * sum|term| of the exact sum, gamma_n =
n u / (1 - n u), u = 2^-24; the rounded difference of L2 adds a relative 2 u per term.  (dim + 2) * 2^-23 * sum|term| is more than
twice that for every dim used here: derived, not measured.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ivf_ref as R  # noqa: E402
from binary_quant_ref import binary_encode_reference  # noqa: E402
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

L2, IP = "SquaredEuclidean", "InnerProduct"
IDX_NONE = 0xffffffff
MAX_KC = 128


def kc_of(topk, refine):
    return min(topk * refine, MAX_KC)


def dim_bits(dim):
    return (dim + 31) // 32 * 32


# ---- scores -----------------------------------------------------------------------------------------------------------------------
def fp64_scores(rows, q, metric):
    """float64 [nq][n]: squared L2, or minus the inner product"""
    r, x = np.asarray(rows, np.float64), np.asarray(q, np.float64)
    if metric == IP:
        return -(x @ r.T)
    return ((x[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)


def band(rows, q, metric):
    """float64 [nq][n]: how far an fp32 score may lie from fp64_scores"""
    r, x = np.asarray(rows, np.float64), np.asarray(q, np.float64)
    mag = np.abs(x) @ np.abs(r).T if metric == IP else ((x[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)
    return (r.shape[1] + 2) * 2.0 ** -23 * mag


# ---- stage 1 ----------------------------------------------------------------------------------------------------------------------
def check_stage1(pos, ham, cnt, cent, offs, bit_rows, qbits, kc, nprobe, max_scan=0xffffffff, exclude=None, what=""):
    """the rule of Hamming lists on the candidates read back (positions are the keys): every candidate probed under model(...),
    admissible and listed once; scores exact and ascending; every admissible probed row strictly below the kc-th candidate's score
    present; count = min(kc, admissible probed rows).  Every query is checked."""
    _, _, _, adm = R.model(cent, offs, qbits, nprobe, max_scan, exclude)
    ref = hamming_reference(bit_rows, qbits) if bit_rows.shape[0] else np.zeros((qbits.shape[0], 0), np.int64)
    assert pos.shape == (qbits.shape[0], kc) and cnt.shape == (qbits.shape[0],)
    check_hamming_lists(pos.astype(np.uint64), ham, cnt, ref, kc, admissible=adm, what=what + " stage 1")


def model_candidates(cent, offs, bit_rows, qbits, kc, nprobe, max_scan=0xffffffff, exclude=None):
    """one valid stage 1: the kc best admissible rows by (Hamming score, position).  (positions [nq][kc], counts [nq])"""
    _, _, _, adm = R.model(cent, offs, qbits, nprobe, max_scan, exclude)
    ref = hamming_reference(bit_rows, qbits)
    pos = np.full((qbits.shape[0], kc), IDX_NONE, np.uint32)
    cnt = np.zeros(qbits.shape[0], np.uint32)
    for i in range(qbits.shape[0]):
        rows = np.nonzero(adm[i])[0]
        rows = rows[np.argsort(ref[i, rows], kind="stable")][:kc]
        pos[i, :rows.size] = rows
        cnt[i] = rows.size
    return pos, cnt


# ---- stage 2 ----------------------------------------------------------------------------------------------------------------------
def stage2_exact(pos, cnt, rows, q, metric, topk, threshold=None, keys=None):
    """the answer on integer-valued data, where every fp32 sum is exact: per query (keys, float32 scores) of the topk smallest by
    (score, candidate rank), then the radius cut"""
    out = []
    for i in range(q.shape[0]):
        c = pos[i, :int(cnt[i])].astype(np.int64)
        s = fp64_scores(rows[c], q[i:i + 1], metric)[0].astype(np.float32)
        assert np.array_equal(s.astype(np.float64), fp64_scores(rows[c], q[i:i + 1], metric)[0]), "not integer data"
        order = np.argsort(s, kind="stable")[:topk]
        if threshold is not None:
            order = order[s[order] <= np.float32(threshold)]
        k = c[order].astype(np.uint64)
        out.append((k if keys is None else np.asarray(keys, np.uint64)[c[order]], s[order]))
    return out


def check_stage2_exact(got_keys, got_scores, got_counts, pos, cnt, rows, q, metric, topk, threshold=None, keys=None, what=""):
    """keys in order, score BITS and counts equal stage2_exact"""
    want = stage2_exact(pos, cnt, rows, q, metric, topk, threshold, keys)
    for i, (wk, ws) in enumerate(want):
        c = int(got_counts[i])
        assert c == wk.size, "%s query %d: count %d, expected %d" % (what, i, c, wk.size)
        assert np.array_equal(np.asarray(got_keys[i, :c], np.uint64), wk), "%s query %d: keys %r, expected %r" % (what, i, got_keys[i, :c], wk)
        assert np.array_equal(np.asarray(got_scores[i, :c], np.float32).view(np.uint32), ws.view(np.uint32)), \
            "%s query %d: scores %r, expected %r" % (what, i, got_scores[i, :c], ws)


def ambiguous_cut(s64, b, topk, threshold=None):
    """does the fp64 reference itself leave the answer open: the two scores at the cut differ by no more than the sum of their bands,
    or a score lies within its band of the radius.  s64 / b: the candidates' scores and bands."""
    order = np.argsort(s64, kind="stable")
    if order.size > topk:
        a, z = order[topk - 1], order[topk]
        if s64[z] - s64[a] <= b[a] + b[z]:
            return True
    if threshold is not None:
        head = order[:topk]
        if np.any(np.abs(s64[head] - threshold) <= b[head]):
            return True
    return False


def check_stage2_real(got_keys, got_scores, got_counts, pos, cnt, rows, q, metric, topk, threshold=None, keys=None, what=""):
    """every returned score within the band of its fp64 score, scores ascending, no duplicate, only candidates; the returned set
    equals the fp64 top-topk of the candidates (then the radius) unless ambiguous_cut.  Returns the number of ambiguous queries."""
    ambiguous = 0
    for i in range(q.shape[0]):
        c = pos[i, :int(cnt[i])].astype(np.int64)
        s64 = fp64_scores(rows[c], q[i:i + 1], metric)[0]
        b = band(rows[c], q[i:i + 1], metric)[0]
        ckeys = c.astype(np.uint64) if keys is None else np.asarray(keys, np.uint64)[c]
        where = {int(k): j for j, k in enumerate(ckeys)}
        n = int(got_counts[i])
        gk = [int(x) for x in got_keys[i, :n]]
        gs = np.asarray(got_scores[i, :n], np.float64)
        assert len(set(gk)) == n and all(k in where for k in gk), "%s query %d: keys %r are not distinct candidates" % (what, i, gk)
        assert np.all(np.diff(gs) >= 0), "%s query %d: scores %r do not ascend" % (what, i, gs)
        for k, s in zip(gk, gs):
            j = where[k]
            assert abs(s - s64[j]) <= b[j], "%s query %d: key %d scored %r, fp64 %r, band %r" % (what, i, k, s, s64[j], b[j])
        if threshold is not None:
            assert np.all(np.asarray(got_scores[i, :n], np.float32) <= np.float32(threshold)), "%s query %d: beyond the radius" % (what, i)
        if ambiguous_cut(s64, b, topk, threshold):
            ambiguous += 1
            assert n <= min(topk, c.size)
            continue
        order = np.argsort(s64, kind="stable")[:topk]
        if threshold is not None:
            order = order[s64[order] <= threshold]
        assert set(gk) == set(int(ckeys[j]) for j in order), "%s query %d: keys %r, expected %r" % (what, i, gk, ckeys[order])
    return ambiguous


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def mask_pad(words, dim):
    """the bits of a row beyond `dim` are 0, as the encoder leaves them"""
    out = np.array(words, np.uint32, copy=True)
    if dim % 32:
        out[:, -1] &= np.uint32((1 << (dim % 32)) - 1)
    return out


def floats_of_bits(rng, words, dim, integer):
    """fp32 [n][dim] whose sign bits (value >= 0) are the first `dim` bits of `words`: integers in [-8, 8], or reals"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :dim].astype(bool)
    if integer:
        mag = np.where(bits, rng.integers(0, 9, bits.shape), rng.integers(-8, 0, bits.shape)).astype(np.float32)
    else:
        a = np.abs(rng.standard_normal(bits.shape)) + 1e-3
        mag = np.where(bits, a, -a).astype(np.float32)
    assert np.array_equal(binary_encode_reference(mag), mask_pad(words, dim))
    return mag


def fp_index(rng, dim, lengths, integer, nq=40):
    """(cent, offs, bit_rows, frows, qf, qbits): hamming_ivf_ref.index_of at 32 * ceil(dim / 32) bits with the pad bits cleared, fp32
    rows and nq fp32 queries that encode to the bits; a third of the queries sit near a row"""
    cent, offs, rows = R.index_of(rng, dim_bits(dim), lengths)
    cent, rows = mask_pad(cent, dim), mask_pad(rows, dim)
    qbits = mask_pad(R.bits(rng, nq, dim_bits(dim)), dim)
    near = rng.integers(0, rows.shape[0], nq // 3)
    qbits[:near.size] = rows[near] ^ mask_pad(R.bits(rng, near.size, dim_bits(dim)) & np.uint32(0x00100401), dim)
    return cent, offs, rows, floats_of_bits(rng, rows, dim, integer), floats_of_bits(rng, qbits, dim, integer), qbits


def short_list(rng, dim=100, integer=True):
    """(cent, offs, bit_rows, frows, qf, qbits, list): every query is nearest to the centroid of `list`, which holds 3 rows; with
    nprobe 1 there are fewer candidates than topk = 5"""
    cent, offs, rows = R.index_of(rng, dim_bits(dim), (40, 3, 60, 0, 25))
    cent, rows = mask_pad(cent, dim), mask_pad(rows, dim)
    qbits = np.repeat(cent[1:2], 6, axis=0)
    qbits[:, 0] ^= np.uint32(1) << np.arange(6, dtype=np.uint32)
    return cent, offs, rows, floats_of_bits(rng, rows, dim, integer), floats_of_bits(rng, qbits, dim, integer), qbits, 1


def two_slices(rng, dim=100):
    """(cent, offs, bit_rows, frows, qf, qbits, nprobe, topk, refine, cap): under the byte cap the search needs more than one slice
    whatever the tile runs (hamming_ivf_ref.min_slices with k = kc)"""
    cent, offs, rows = R.index_of(rng, dim_bits(dim), (100, 130, 20, 260, 90))
    cent, rows = mask_pad(cent, dim), mask_pad(rows, dim)
    qbits = mask_pad(R.bits(rng, 7, dim_bits(dim)), dim)
    return cent, offs, rows, floats_of_bits(rng, rows, dim, True), floats_of_bits(rng, qbits, dim, True), qbits, 3, 5, 4, 1024


def max_scan_case(rng, dim=96):
    """hamming_ivf_ref.max_scan_case with fp32 rows and queries: (cent, offs, bit_rows, frows, qf, qbits, nprobe, length)"""
    cent, offs, rows, q, nprobe, length = R.max_scan_case(rng, dim)
    return cent, offs, rows, floats_of_bits(rng, rows, dim, True), floats_of_bits(rng, q, dim, True), q, nprobe, length
