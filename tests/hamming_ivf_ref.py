"""Model of the Hamming IVF index (numpy only; nothing here touches the GPU or the library): the probe order, the max-scan cut, the
rows a search may return, the trainer's labelling and majority step, the seeded choice of the initial centroids, and the fixtures
of tests/test_gpu_hamming_ivf.py.  tests/test_hamming_ivf_reference_cpu.py pins the model by hand and holds every fixture to the
preconditions that keep a GPU test from passing vacuously.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hamming_ref import hamming_reference  # noqa: E402


def bits(rng, n, dim, dtype="binary32"):
    words = rng.integers(0, 2**32, (n, dim // 32), dtype=np.uint64).astype(np.uint32)
    return words if dtype == "binary32" else np.ascontiguousarray(words).view(np.uint64)


def probe_order(cent, q, nprobe):
    """uint32 [nq][min(nprobe, nlist)]: the centroids smallest by the pair (distance, centroid index), ascending"""
    d = hamming_reference(cent, q)
    key = d * (1 << 32) + np.arange(cent.shape[0], dtype=np.int64)[None, :]
    return np.argsort(key, axis=1, kind="stable")[:, :min(nprobe, cent.shape[0])].astype(np.uint32)


def max_scan_cut(order, offs, max_scan):
    """probe list i while the running scanned count is < max_scan, adding the list's length after each probe:
    (probe_cnt [nq], scanned [nq])"""
    offs = np.asarray(offs, np.int64)
    cnt = np.zeros(order.shape[0], np.uint32)
    scanned = np.zeros(order.shape[0], np.uint32)
    for i, row in enumerate(order):
        total = 0
        for l in row:
            if not total < max_scan:
                break
            cnt[i] += 1
            total += int(offs[l + 1] - offs[l])
        scanned[i] = total
    return cnt, scanned


def admissible(order, cnt, offs, exclude=None):
    """bool [nq][n]: the union of the probed lists, minus the excluded positions (exclude: bool [n])"""
    offs = np.asarray(offs, np.int64)
    adm = np.zeros((order.shape[0], int(offs[-1])), bool)
    for i, row in enumerate(order):
        for l in row[:cnt[i]]:
            adm[i, offs[l]:offs[l + 1]] = True
    if exclude is not None:
        adm &= ~np.asarray(exclude, bool)[None, :]
    return adm


def model(cent, offs, q, nprobe, max_scan, exclude=None):
    order = probe_order(cent, q, nprobe)
    cnt, scanned = max_scan_cut(order, offs, max_scan)
    return order, cnt, scanned, admissible(order, cnt, offs, exclude)


def labels(cent, rows):
    """the nearest centroid of every row by (distance, index)"""
    return probe_order(cent, rows, 1)[:, 0]


def majority_step(cent, rows, lab):
    """every centroid with members becomes their bitwise majority: bit i set iff ones_i > (members >> 1); one without keeps its bits"""
    out = np.array(cent, copy=True)
    rb = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], -1), axis=1, bitorder="little")
    for l in range(cent.shape[0]):
        mem = rb[lab == l]
        if mem.shape[0] == 0:
            continue
        maj = (mem.sum(axis=0, dtype=np.int64) > (mem.shape[0] >> 1)).astype(np.uint8)
        out[l] = np.packbits(maj, bitorder="little").view(cent.dtype)
    return out


def initial_rows(n, nlist, seed):
    """nlist distinct row numbers: a partial Fisher-Yates shuffle driven by splitmix64(seed), draws reduced by % (n - i)"""
    mask = (1 << 64) - 1
    state = seed & mask
    place = {}
    out = []
    for i in range(nlist):
        state = (state + 0x9e3779b97f4a7c15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        z ^= z >> 31
        j = i + z % (n - i)
        vi, vj = place.get(i, i), place.get(j, j)
        out.append(vj)
        place[j] = vi
    return np.asarray(out, np.int64)


def words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def min_slices(count, np_, k, cap):
    """slices a search of `count` queries needs AT LEAST under the byte cap: a query's partial lists take np * k * 8 bytes per tile
    run, and there is at least one run"""
    return -(-count // max(1, cap // (np_ * k * 8)))


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
RAGGED = (0, 1, 127, 128, 129, 300)       # lists that start and end off the tile grid; the last spans three tiles


def index_of(rng, dim, lengths, dtype="binary32"):
    """(centroids, offsets, rows): random centroids, every list's rows within dim // 8 flipped bits of its centroid"""
    nlist = len(lengths)
    cent = bits(rng, nlist, dim)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    rows = np.repeat(cent, lengths, axis=0)
    flips = np.zeros((rows.shape[0], dim), np.uint8)
    for r in range(rows.shape[0]):
        flips[r, rng.choice(dim, rng.integers(0, dim // 8 + 1), replace=False)] = 1
    rows = rows ^ np.packbits(flips, axis=1, bitorder="little").view(np.uint32)
    if dtype == "binary64":
        cent, rows = np.ascontiguousarray(cent).view(np.uint64), np.ascontiguousarray(rows).view(np.uint64)
    return cent, offs, rows


def duplicate_centroids(rng, dim=96):
    """centroid 3 repeats centroid 1, and every query is nearest to that pair: with nprobe 1 the tie is AT the probe boundary"""
    cent, offs, rows = index_of(rng, dim, (40, 50, 60, 70, 30))
    cent[3] = cent[1]
    q = np.repeat(cent[1:2], 9, axis=0)
    q[:, 0] ^= np.uint32(1) << np.arange(9, dtype=np.uint32)          # one flipped bit each: distance 1 to both
    return cent, offs, rows, q


def crowded_lists(rng, nq, dim=96):
    """two lists and nprobe 2: each list is probed by all nq queries"""
    cent, offs, rows = index_of(rng, dim, (200, 150))
    return cent, offs, rows, bits(rng, nq, dim)


def two_slices(rng, dim=96):
    """(cent, offs, rows, q, nprobe, k, cap): under the byte cap `cap` the search needs more than one slice whatever the tile runs"""
    cent, offs, rows = index_of(rng, dim, (100, 130, 20, 260, 90))
    return cent, offs, rows, bits(rng, 7, dim), 3, 10, 1024


def max_scan_case(rng, dim=96):
    """(cent, offs, rows, q, nprobe, length): `length` is the length of the list query 0 probes first, and it is not empty"""
    cent, offs, rows = index_of(rng, dim, RAGGED)
    q = cent[[3, 5, 2, 4, 1, 0]] ^ bits(rng, 6, dim) & np.uint32(0x00010001)      # near one centroid each; query 0 near list 3
    first = int(probe_order(cent, q, 1)[0, 0])
    return cent, offs, rows, q, 4, int(offs[first + 1] - offs[first])
