"""The cases of tests/test_gpu_sparse_put_dev.py (zvec_hip_sparse_put_dev), as data, and the plan a put makes of a call, in plain
Python over the model of tests/sparse_put_ref.py.  numpy only: tests/test_sparse_put_dev_reference_cpu.py holds every case to what it
claims (the routes, the chunk boundaries, the parities, the dropped rows) without a GPU, so a case that drifts fails there instead of
quietly testing nothing on the device.

A case is a list of steps.  A step is a dict:
    kind    "put" (one zvec_hip_sparse_put_dev on the handle, one zvec_hip_sparse_put of the same arrays on its twin) or "append"
            (zvec_hip_sparse_append on both)
    ids, rows, keys     the call: rows is a list of (indices, values); keys None or a list
    route   the route the step claims: 0 tail, 1 in place, 2 splice (puts only)
    src_off the caller's d_indices / d_values start this many elements into a larger device tensor (puts only)
"""
import numpy as np

import sparse_put_ref as M

VOCAB = 6000
BASE = [5, 9, 0, 7, 12, 3, 30, 1]


def put(ids, rows, route, keys=None, src_off=0):
    return {"kind": "put", "ids": [int(i) for i in ids], "rows": rows, "keys": keys, "route": route, "src_off": src_off}


def append(rows):
    return {"kind": "append", "rows": rows}


def rows_of(rng, lengths, dtype, vocab=VOCAB):
    """random rows; those of a small vocabulary are searched and carry no denormals"""
    return [M.random_row(rng, c, vocab, M.NP[dtype], specials=vocab == VOCAB) for c in lengths]


def apply_step(model, step):
    """the step on the model"""
    counts, idx, val = M.pack(step["rows"], model.np_dtype)
    if step["kind"] == "append":
        n0 = model.count()
        M.apply_put(model, np.arange(n0, n0 + len(counts)), counts, idx, val)
    else:
        M.apply_put(model, step["ids"], counts, idx, val, step["keys"])


def plan(model, step):
    """What a put makes of the call on a store that holds `model`, following csrc/host/sparse_put_plan.h: the kept rows (the last one
    of every id) ascending by id, as numbers of the call's rows; the route; per overwritten row the running shift (new minus old
    pairs up to and including it); per kept row with pairs the parity of (its place in the stage - its place in the caller's
    array), src_off included: 0 where a half keeps its place in a 32-bit word on the way into the stage, 1 where it changes it."""
    ids = step["ids"]
    counts = [len(r[0]) for r in step["rows"]]
    old_n = model.count()
    last = {}
    for i, d in enumerate(ids):
        last[d] = i
    keep = [last[d] for d in sorted(last)]
    over = [i for i in keep if ids[i] < old_n]
    same = all(counts[i] == model.rows[ids[i]][0].size for i in over)
    in_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sb, shifts, shift, stage_par = 0, [], 0, []
    for i in keep:
        if counts[i]:
            stage_par.append(int((sb - (in_off[i] + step["src_off"])) & 1))
        sb += counts[i]
        if ids[i] < old_n:
            shift += counts[i] - int(model.rows[ids[i]][0].size)
            shifts.append(shift)
    return {"keep": keep, "dropped": sorted(set(range(len(ids))) - set(keep)), "route": 0 if not over else 1 if same else 2,
            "shifts": shifts, "stage_parities": stage_par, "descending": all(a >= b for a, b in zip(ids, ids[1:])) and len(ids) > 1}


def offsets(model):
    return np.concatenate([[0], np.cumsum([r[0].size for r in model.rows])]).astype(np.int64)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def case_tail(dtype):
    """ids at and behind the count with gaps, a put into one of the holes, a host append on top (the hole bits grow past their first
    word), and a put behind the appended rows"""
    rng = np.random.default_rng([21, int(dtype == "fp16")])
    return [
        put([0, 1, 2, 5, 9], rows_of(rng, [5, 0, 17, 64, 3], dtype), 0),
        put([12, 10], rows_of(rng, [65, 4096], dtype), 0, keys=[912, 910]),
        put([4], rows_of(rng, [6], dtype), 2),                    # a hole stops being one (it held no pairs: the splice)
        put([7], rows_of(rng, [0], dtype), 1),                    # ... and an empty row over a hole keeps its length
        append(rows_of(rng, [3, 0, 8] * 30, dtype)),
        put([110, 103], rows_of(rng, [2, 9], dtype), 0),
    ]


def case_in_place(dtype):
    rng = np.random.default_rng([22, int(dtype == "fp16")])
    lengths = [7, 0, 33, 1, 64, 4096, 2, 65, 12, 5]
    ids = [7, 1, 5, 2, 3]
    return [
        put(range(len(lengths)), rows_of(rng, lengths, dtype), 0),
        put(ids, rows_of(rng, [lengths[i] for i in ids], dtype), 1, keys=[507, 501, 505, 502, 503]),
        put([4, 10, 12], rows_of(rng, [64, 3, 8], dtype), 1),      # with rows behind the old end in the same call
    ]


def case_splice(dtype, chunk):
    """A store of a little over 3 * chunk pairs in rows of about 100.  Row a ends exactly on the first chunk boundary, row b one pair
    in front of the second, row c one pair behind the third.  Returns (steps, (a, b, c)).  Step 1 replaces the three by rows one
    longer, one shorter, one longer (net +1: everything behind c moves by an odd count); step 2, ids descending, by rows one shorter
    each (running shifts -1, -2: odd and even); step 3 puts b back (+1)."""
    rng = np.random.default_rng([23, int(dtype == "fp16")])
    lengths, marks, at = [], [], 0
    for target in (chunk, 2 * chunk - 1, 3 * chunk + 1):
        while target - at > 150:
            lengths.append(100)
            at += 100
        lengths.append(target - at)                               # (51 .. 150 pairs)
        at = target
        marks.append(len(lengths) - 1)
    lengths.append(49)
    a, b, c = marks
    la, lb, lc = lengths[a], lengths[b], lengths[c]
    steps = [
        put(range(len(lengths)), rows_of(rng, lengths, dtype), 0),
        put([a, b, c], rows_of(rng, [la + 1, lb - 1, lc + 1], dtype), 2),
        put([c, b], rows_of(rng, [lc, lb - 2], dtype), 2),
        put([b], rows_of(rng, [lb - 1], dtype), 2),
    ]
    return steps, (a, b, c)


ALIGN_LENGTHS = [1, 2, 3, 63, 64, 65, 257]


def case_alignment(dtype, src_off):
    """rows of 1, 2, 3, 63, 64, 65 and 257 pairs back to back in a view that starts src_off elements into a larger tensor: a tail
    put, the same ids in place, and the ids descending with every length changed by one (the splice)"""
    rng = np.random.default_rng([24, int(dtype == "fp16"), src_off])
    n = len(ALIGN_LENGTHS)
    changed = [c + (1 if i % 2 else -1) for i, c in enumerate(ALIGN_LENGTHS)]
    return [
        put(range(n), rows_of(rng, ALIGN_LENGTHS, dtype), 0, src_off=src_off),
        put(range(n), rows_of(rng, ALIGN_LENGTHS, dtype), 1, src_off=src_off),
        put(range(n - 1, -1, -1), rows_of(rng, changed[::-1], dtype), 2, src_off=src_off),
    ]


def case_keep_last(dtype):
    """an id named three times in one call with rows of different lengths, the ids descending, on each route"""
    rng = np.random.default_rng([25, int(dtype == "fp16")])
    n = len(BASE)
    return [
        put(range(n), rows_of(rng, BASE, dtype), 0),
        put([9, 6, 4, 4, 4, 2], rows_of(rng, [3, 5, 2, 9, 6, 1], dtype), 2, keys=[19, 16, 141, 142, 143, 12]),
        put([5, 5, 5, 1], rows_of(rng, [7, 1, BASE[5], BASE[1]], dtype), 1),
        put([14, 14, 14, 12], rows_of(rng, [4, 0, 11, 2], dtype), 0),
    ]


def case_search(dtype, metric):
    """a mixed sequence of the three routes over a small vocabulary, and queries for it: (steps, queries)"""
    import sparse_ref as R
    rng = np.random.default_rng([26, int(dtype == "fp16"), int(metric == "InnerProductSparse")])
    vocab = 60
    lens = [int(c) for c in rng.choice([0, 1, 8, 20], 300)]
    ids = [int(i) for i in rng.choice(300, 40, replace=False)]
    new = [int(c) for c in rng.choice([0, 3, 25], 40)]
    new[0] = lens[ids[0]] + 1                                     # (a changed length for certain)
    steps = [
        put(range(300), rows_of(rng, lens, dtype, vocab), 0),
        put([320, 305, 340], rows_of(rng, [9, 4, 12], dtype, vocab), 0, keys=[9320, 9305, 9340]),
        put(ids, rows_of(rng, new, dtype, vocab), 2),
        put(ids[:10], rows_of(rng, new[:10], dtype, vocab), 1),
        put([310, 7, 345, 7], rows_of(rng, [6, 2, 3, 30], dtype, vocab), 2),
    ]
    queries = R.random_runs(rng, rng.choice([0, 1, 10, 40], 9), vocab)
    return steps, (queries[0], queries[1], queries[2].astype(M.NP[dtype]))
