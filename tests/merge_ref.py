"""Reference of the merge / select step (merge_kernel, zvec_amd/csrc/zvk_merge.hip.h): a numpy model of its CONTRACT, not of the kernel.

The rule.  One query's candidates are records (score, slot, entry, valid, key).  Keep the valid ones with score <= threshold, order
them by (score, slot, entry) with a stable sort — or by (score, ordinal) for streams merged in stream order — emit the first k, and
pad the tail with key ~0 and score +inf; count = the number emitted.  The model does no arithmetic, so every comparison with the GPU
is exact.  Scores compare by VALUE (-0.0 == +0.0): one path of the kernel canonicalises the sign of zero and another does not, and
that is not part of the contract.  Inputs never hold NaN, nor +inf as a real score.

From one candidate table the builders below make the layouts the entries take: strided [part][q][k] arrays with counts, the packed
per-part buffer of zvec_hip_packed_bytes with a chosen part stride, and per-query position lists.  The case tables are shared by
test_merge_reference_cpu.py and test_gpu_merge.py.
"""
import collections
import zlib

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
KEY_NONE = 0xffffffffffffffff
IDX_NONE = 0xffffffff

# merge_kernel sorts up to SURV = 128 survivors at once and gathers up to GATHER = 512 (zvk_merge.hip.h, `constexpr uint32_t SURV`
# / `GATHER`); quoted here once, for expected_path only
SORT_MAX, GATHER_MAX = 128, 512

PATHS = ("sort", "trim", "general-overflow", "general-ties", "general-k")

# one query's candidates, in stream order: score f32, slot u32, entry u32, valid bool, key u64 — arrays of one length
Cands = collections.namedtuple("Cands", "score slot entry valid key")


def _rng(*name):
    return np.random.default_rng(zlib.crc32(repr(name).encode()))


# ---- the rule ---------------------------------------------------------------------------------
def merge_model(c, k, threshold=FLT_MAX, ordinal=False):
    """(keys [k] u64, scores [k] f32, count) of one query's candidates `c`"""
    keep = np.nonzero(c.valid & (c.score <= np.float32(min(threshold, FLT_MAX))))[0]
    if ordinal:
        order = keep[np.argsort(c.score[keep], kind="stable")]                  # keep is ascending: ties stay in stream order
    else:
        order = keep[np.lexsort((c.entry[keep], c.slot[keep], c.score[keep]))]    # (lexsort is stable; the last key is the primary one)
    order = order[:k]
    keys = np.full(k, KEY_NONE, np.uint64)
    scores = np.full(k, np.inf, np.float32)
    keys[:order.size] = c.key[order]
    scores[:order.size] = c.score[order]
    return keys, scores, int(order.size)


def merge_model_batch(table, k, threshold=FLT_MAX, ordinal=False):
    """the rule for every query of a table (a list of Cands): keys [nq][k], scores [nq][k], counts [nq]"""
    rows = [merge_model(c, k, threshold, ordinal) for c in table]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.asarray([r[2] for r in rows], np.uint32))


def assert_same(got, want, what=""):
    """exact equality of keys, counts and score VALUES, the padded tail included"""
    gk, gs, gc = got
    wk, ws, wc = want
    assert np.asarray(gc).astype(np.int64).tolist() == np.asarray(wc).astype(np.int64).tolist(), "%s: counts" % what
    gk, wk = np.asarray(gk).astype(np.uint64), np.asarray(wk).astype(np.uint64)
    gs, ws = np.asarray(gs, np.float32), np.asarray(ws, np.float32)
    assert gk.shape == wk.shape and gs.shape == ws.shape, "%s: shapes" % what
    if not np.array_equal(gk, wk):
        q, j = np.argwhere(gk != wk)[0]
        raise AssertionError("%s: key [%d][%d] = %d, expected %d (score %r, expected %r)" % (what, q, j, gk[q, j], wk[q, j], gs[q, j], ws[q, j]))
    if not np.array_equal(gs, ws):                   # (by value: -0.0 == +0.0, +inf == +inf; there is no NaN)
        q, j = np.argwhere(gs != ws)[0]
        raise AssertionError("%s: score [%d][%d] = %r, expected %r" % (what, q, j, gs[q, j], ws[q, j]))


def expected_path(c, k, threshold=FLT_MAX):
    """The path of merge_kernel this query is MEANT to take, from the counts the model sees: the admitted candidates A, the
    candidates at or below the k-th admitted score T (every admitted one when fewer than k are), and k.

      k > 128                      general-k          (the survivor paths serve k <= SORT_MAX only)
      A <= 128                     sort
      A > 512                      general-overflow
      129 <= A <= 512, T <= 128    trim               (the bisection keeps k plus ties, then the sort)
      129 <= A <= 512, T > 128     general-ties

    This documents intent; it does not read the kernel.  128 and 512 are SURV and GATHER of zvk_merge.hip.h: whoever changes those
    two constants follows them here (SORT_MAX, GATHER_MAX) by hand.  A pre-bound (k <= 64 over a dense row or over >= 64 slot heads)
    can only lower the survivors below A, towards `sort`: see bound_is_moot."""
    if k > SORT_MAX:
        return "general-k"
    s = np.sort(c.score[c.valid & (c.score <= np.float32(min(threshold, FLT_MAX)))])
    a = s.size
    if a <= SORT_MAX:
        return "sort"
    if a > GATHER_MAX:
        return "general-overflow"
    t = a if a < k else int(np.count_nonzero(s <= s[k - 1]))
    return "trim" if t <= SORT_MAX else "general-ties"


def bound_is_moot(c, k, threshold=FLT_MAX, stream_len=None):
    """True when no pre-bound of the kernel can take a survivor away from this query, so that expected_path is the path taken:
    k > 64 or a stream shorter than 64 (no bound is computed), fewer than k admissible candidates (the bound is +inf or the
    threshold), or every admitted score equal (the bound is that score)."""
    n = c.score.size if stream_len is None else stream_len
    s = c.score[c.valid & (c.score <= np.float32(min(threshold, FLT_MAX)))]
    return k > 64 or n < 64 or s.size < k or bool(np.all(s == s[0]))


# ---- layouts ----------------------------------------------------------------------------------
def to_strided(table, nparts, k):
    """keys u64 / scores f32 [nparts][nq][k] and counts u32 [nparts][nq] of a table whose slot = part and entry = place in the part's
    list (the valid entries of a part are its first ones).  What lies beyond a part's count is poisoned with the best score there
    is and a key of its own: an entry that ignores the counts shows."""
    nq = len(table)
    keys = np.full((nparts, nq, k), 0xdead0000dead, np.uint64)
    scores = np.full((nparts, nq, k), -FLT_MAX, np.float32)
    counts = np.zeros((nparts, nq), np.uint32)
    for q, c in enumerate(table):
        assert np.all(c.valid) and np.all(c.entry < k) and np.all(c.slot < nparts)
        keys[c.slot, q, c.entry] = c.key
        scores[c.slot, q, c.entry] = c.score
        np.add.at(counts[:, q], c.slot, 1)
        assert np.all(c.entry < counts[c.slot, q])                       # entries 0 .. count - 1 of every part, each once
    return keys, scores, counts


def from_strided(keys, scores, counts):
    """the table of strided shard lists (the inverse of to_strided)"""
    nparts, nq, k = keys.shape
    table = []
    for q in range(nq):
        slot = np.repeat(np.arange(nparts, dtype=np.uint32), counts[:, q])
        entry = np.concatenate([np.arange(n, dtype=np.uint32) for n in counts[:, q]] + [np.zeros(0, np.uint32)])
        table.append(Cands(scores[slot, q, entry].astype(np.float32), slot, entry, np.ones(slot.size, bool), keys[slot, q, entry].astype(np.uint64)))
    return table


def packed_bytes(nq, k):
    """zvec_hip_packed_bytes: [nq * k keys u64][nq * k scores f32][nq counts u32], padded to 16 bytes"""
    return (nq * k * 12 + nq * 4 + 15) // 16 * 16


def to_packed(keys, scores, counts, part_stride):
    """the all-gather buffer: part p's three arrays start p * part_stride bytes in; the padding holds 0xa5"""
    nparts, nq, k = keys.shape
    assert part_stride >= packed_bytes(nq, k) and part_stride % 8 == 0
    buf = np.full(nparts * part_stride, 0xa5, np.uint8)
    for p in range(nparts):
        o = p * part_stride
        buf[o:o + nq * k * 8] = np.ascontiguousarray(keys[p]).view(np.uint8).reshape(-1)
        buf[o + nq * k * 8:o + nq * k * 12] = np.ascontiguousarray(scores[p]).view(np.uint8).reshape(-1)
        buf[o + nq * k * 12:o + nq * k * 12 + nq * 4] = np.ascontiguousarray(counts[p]).view(np.uint8).reshape(-1)
    return buf


def position_lists(table):
    """per-query position lists of a table whose entry (flat by-positions) or key (sparse by-ids) is the listed position"""
    return [c.entry.astype(np.uint32) for c in table]


# ---- A. shard lists ---------------------------------------------------------------------------
# name, nq, k, valid candidates per query, counts pattern, score pattern
#   counts: full (n = parts x k) / zero / one (one part of four holds everything, n <= k) / ragged (n dealt over ceil(n / k) + 2 parts,
#   differently for every query)
#   scores: distinct / equal / tieN_B (exactly N candidates share the k-th score, B better ones in front of them) / negative / zeros
#   (+-0 and +-1) / fltmax (+-FLT_MAX among small values) / denormal / dupkey (distinct scores, the same key in two parts)
ShardCase = collections.namedtuple("ShardCase", "name nq k n counts scores")
SHARD_CASES = [ShardCase("%s-q%d-k%d-n%d" % (s, nq, k, n), nq, k, n, cnt, s) for (nq, k, n, cnt, s) in [
    (1, 10, 0, "zero", "distinct"), (65, 129, 0, "zero", "distinct"),
    (1, 1, 1, "one", "distinct"), (65, 10, 1, "ragged", "distinct"), (1, 300, 1, "one", "equal"),
    (1, 10, 127, "ragged", "distinct"), (65, 128, 127, "one", "zeros"), (1, 64, 128, "full", "distinct"),
    (65, 65, 128, "ragged", "equal"), (1, 128, 128, "one", "fltmax"), (1, 129, 129, "full", "distinct"),
    (65, 10, 129, "ragged", "distinct"), (1, 65, 129, "ragged", "negative"), (1, 1, 129, "full", "denormal"),
    (1, 128, 511, "ragged", "distinct"), (65, 64, 512, "full", "dupkey"), (1, 10, 512, "ragged", "zeros"),
    (1, 1, 513, "full", "distinct"), (65, 65, 513, "ragged", "fltmax"), (1, 128, 2000, "ragged", "distinct"),
    (65, 10, 2000, "ragged", "negative"), (1, 64, 2000, "ragged", "equal"), (1, 300, 2000, "ragged", "dupkey"),
    (65, 300, 513, "ragged", "equal"), (1, 129, 2000, "ragged", "denormal"), (1, 300, 300, "one", "distinct"),
    # exactly 128 / 129 candidates at the k-th score: the last list one sort takes, the first it does not
    (1, 1, 300, "ragged", "tie128_0"), (1, 1, 300, "ragged", "tie129_0"), (65, 10, 511, "ragged", "tie128_0"), (65, 10, 511, "ragged", "tie129_0"),
    (1, 10, 300, "ragged", "tie119_9"), (1, 10, 300, "ragged", "tie120_9"), (1, 64, 512, "full", "tie128_60"), (1, 128, 512, "ragged", "tie129_100"),
    (1, 65, 300, "ragged", "equal"), (65, 128, 300, "ragged", "distinct"), (1, 10, 2000, "ragged", "tie129_3"),
]]


def _shard_scores(rng, pattern, n, k):
    if pattern in ("distinct", "dupkey"):
        return (rng.permutation(n) - n // 3).astype(np.float32)
    if pattern == "equal":
        return np.full(n, 7.0, np.float32)
    if pattern == "negative":
        return (-1.0 - rng.permutation(n)).astype(np.float32) * np.float32(0.25)
    if pattern == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), n)
    if pattern == "fltmax":
        return rng.choice(np.array([FLT_MAX, -FLT_MAX, 0.0, 3.0, -3.0], np.float32), n)
    if pattern == "denormal":
        return (rng.integers(-40, 41, n).astype(np.int64) // 2).astype(np.float32) * np.float32(1.4e-45) + np.float32(0.0)
    assert pattern.startswith("tie")
    tied, better = (int(x) for x in pattern[3:].split("_"))
    assert better < k <= better + tied <= n
    s = np.concatenate([-1.0 - np.arange(better), np.zeros(tied), 1.0 + rng.permutation(n - better - tied)]).astype(np.float32)
    return s[rng.permutation(n)]


def _shard_counts(rng, pattern, n, k):
    if pattern == "zero":
        assert n == 0
        return np.zeros(3, np.int64)
    if pattern == "one":
        assert n <= k
        return np.array([0, 0, n, 0], np.int64)
    if pattern == "full":
        assert n and n % k == 0
        return np.full(n // k, k, np.int64)
    nparts = (n + k - 1) // k + 2
    return rng.multivariate_hypergeometric(np.full(nparts, k), n)


def shard_case(case):
    """(table, nparts) of a ShardCase; slot = part, entry = place in the part's list"""
    table, nparts = [], None
    for q in range(case.nq):
        rng = _rng(case.name, q)
        cnt = _shard_counts(rng, case.counts, case.n, case.k)
        nparts = cnt.size
        slot = np.repeat(np.arange(nparts, dtype=np.uint32), cnt)
        entry = np.concatenate([np.arange(c, dtype=np.uint32) for c in cnt] + [np.zeros(0, np.uint32)])
        key = rng.permutation(case.n).astype(np.uint64) * np.uint64(0x100000001) + np.uint64(5)       # distinct, most beyond 32 bits
        if case.scores == "dupkey" and case.n:
            first = np.nonzero(slot == slot[0])[0]
            other = np.nonzero(slot == slot[-1])[0][:first.size]
            key[other] = key[first[:other.size]]                        # the same keys in two parts: both are candidates, both are kept
        table.append(Cands(_shard_scores(rng, case.scores, case.n, case.k), slot, entry, np.ones(case.n, bool), key))
    return table, nparts


# ---- B / C. position lists --------------------------------------------------------------------
# Rows whose score from the query below is a chosen integer.  STORE_ROWS rows: [0, 1024) score r // 2 (pairs tie), [1024, 1724) all
# score 500 (ties with rows 1000 and 1001), [1724, 2048) descending, so that position order is not score order.
STORE_ROWS = 2048
TIED_ROWS = (1024, 1724)
TIED_SCORE = 500


def chosen_scores():
    r = np.arange(STORE_ROWS)
    return np.where(r < 1024, r // 2, np.where(r < TIED_ROWS[1], TIED_SCORE, 2600 - r)).astype(np.int64)


def store_keys():
    return np.arange(STORE_ROWS, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33)


def flat_rows():
    """[2048][4] fp32 rows of integers |v| <= 64 whose squared norm is chosen_scores() (four squares), signs mixed"""
    best = {}
    for a in range(30):
        for b in range(a + 1):
            for c in range(b + 1):
                for d in range(c + 1):
                    best.setdefault(a * a + b * b + c * c + d * d, (a, b, c, d))
    rows = np.array([best[int(s)] for s in chosen_scores()], np.float32)
    assert np.abs(rows).max() <= 64
    return rows * np.where(_rng("signs").random(rows.shape) < 0.5, -1, 1).astype(np.float32)


# sparse rows of one term: row r holds term r % 2 with the value v[r]; the query holds term 0 with weight 1 and term 1 with weight 64,
# so the score -(inner product) is -v[r] or -64 v[r]
def sparse_values():
    r = np.arange(STORE_ROWS)
    v = (r * 37 % 129 - 64).astype(np.int64)
    v[TIED_ROWS[0]:TIED_ROWS[1]] = np.where(r[TIED_ROWS[0]:TIED_ROWS[1]] % 2 == 0, -64, -1)       # every tied row scores 64
    return v


def sparse_scores():
    return -(sparse_values() * np.where(np.arange(STORE_ROWS) % 2 == 0, 1, 64))


HOLES = np.array([STORE_ROWS, STORE_ROWS + 5, 1 << 20, 0xffffffff], np.uint32)

# name, list kind, list length, k, threshold ("max" = FLT_MAX, "inf", "below" = under every score, "tied" = exactly the tied score)
ListCase = collections.namedtuple("ListCase", "name kind length k threshold")
LIST_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
LIST_KS = (1, 10, 64, 65, 128, 129)
LIST_CASES = (
    [ListCase("mixed-%d-k%d" % (n, k), "mixed", n, k, "max") for n in LIST_LENGTHS for k in LIST_KS] +
    [ListCase("tied-%d-k%d" % (n, k), "tied", n, k, "max") for n in (100, 300, 600) for k in (10, 64, 65, 128, 129)] +
    [ListCase("%s-%d-k%d-%s" % (kind, n, k, t), kind, n, k, t) for kind, n in (("mixed", 1025), ("tied", 300), ("mixed", 65))
     for k in (10, 128) for t in ("below", "tied", "inf")])

# the variants of one case, one query each: how many of the list's entries are holes
VARIANTS = ("few", "most", "some")


def list_positions(case):
    """the position lists of a case, one per variant: rows drawn with repeats (2049 entries repeat some of 2048 rows anyway), one row
    listed twice in a row's distance, positions beyond the rows sprinkled in — `few`: one in twenty; `most`: all but 7 (fewer valid
    entries than any k > 7); `some`: all but 300 or so of a long list (the range one k-select trims)"""
    lists = []
    for v in VARIANTS:
        rng = _rng(case.name, v)
        lo, hi = TIED_ROWS if case.kind == "tied" else (0, STORE_ROWS)
        pos = rng.integers(lo, hi, case.length).astype(np.uint32)
        if case.length >= 3:
            pos[case.length // 2] = pos[0]                               # a repeated position: returned twice
        hole = np.zeros(case.length, bool)
        if v == "few":
            hole = rng.random(case.length) < 0.05
        elif v == "most":
            hole[rng.permutation(case.length)[7:]] = True
        elif v == "some":
            hole[rng.permutation(case.length)[300:]] = True
        pos[hole] = rng.choice(HOLES, int(hole.sum()))
        lists.append(pos)
    return lists


def list_threshold(case, scores):
    tied = float(TIED_SCORE if scores is None else scores[TIED_ROWS[0]])
    low = float(-1.0 if scores is None else scores.min() - 1)
    return {"max": FLT_MAX, "inf": float("inf"), "below": low, "tied": tied}[case.threshold]


def flat_list_table(lists):
    """flat by-positions: one slot, ties in the order of the POSITIONS (entry = position), key through the store's key map"""
    s, keys = chosen_scores(), store_keys()
    table = []
    for pos in lists:
        ok = pos < STORE_ROWS
        p = np.where(ok, pos, 0)
        table.append(Cands(np.where(ok, s[p], np.inf).astype(np.float32), np.zeros(pos.size, np.uint32), pos.astype(np.uint32), ok,
                           np.where(ok, keys[p], np.uint64(KEY_NONE))))
    return table


def sparse_list_table(lists):
    """sparse by-ids: every listed entry is a slot of its own, ties in LIST order (slot = place in the list)"""
    s, keys = sparse_scores(), store_keys()
    table = []
    for pos in lists:
        ok = pos < STORE_ROWS
        p = np.where(ok, pos, 0)
        table.append(Cands(np.where(ok, s[p], np.inf).astype(np.float32), np.arange(pos.size, dtype=np.uint32), np.zeros(pos.size, np.uint32), ok,
                           np.where(ok, keys[p], np.uint64(KEY_NONE))))
    return table


# ---- D. the IVF small-batch route as a dense-row selector --------------------------------------
# nlist lists of one row each, the row = the centroid: 1-d integers in [-16, 16] with many ties.  topk = nprobe, every probed list is
# scanned: the result is the coarse selection itself, centroids by (score, id).
IvfCase = collections.namedtuple("IvfCase", "name nlist nprobe nq")
IVF_CASES = [IvfCase("nlist%d-nprobe%d" % (nl, np_), nl, np_, 1 + (nl + np_) % 8)
             for nl in (64, 65, 129, 513, 600) for np_ in (1, 64, 65, 128, 129) if np_ < nl]


def ivf_centroids(nlist):
    return ((np.arange(nlist) * 7) % 33 - 16).astype(np.float32).reshape(nlist, 1)


def ivf_keys(nlist):
    return np.arange(nlist, dtype=np.uint64) * np.uint64(5) + np.uint64(100)


def ivf_queries(case):
    return _rng(case.name).integers(-20, 21, (case.nq, 1)).astype(np.float32)


def ivf_table(case):
    """the centroid row of every query as one dense row: entry = centroid id, score = (q - c)^2, exact"""
    cent, keys = ivf_centroids(case.nlist)[:, 0], ivf_keys(case.nlist)
    ids = np.arange(case.nlist, dtype=np.uint32)
    return [Cands(((q - cent) * (q - cent)).astype(np.float32), np.zeros(case.nlist, np.uint32), ids, np.ones(case.nlist, bool), keys)
            for q in ivf_queries(case)[:, 0]]


def ivf_paths(case):
    """the classes of the two selections of a case: the coarse step over the row of nlist scores, the final merge over the nprobe
    scored rows (both with k = nprobe)"""
    out = set()
    for c in ivf_table(case):
        out.add(expected_path(c, case.nprobe))
        top = np.argsort(c.score, kind="stable")[:case.nprobe]
        out.add(expected_path(Cands(c.score[top], c.slot[top], c.entry[top], c.valid[top], c.key[top]), case.nprobe))
    return out
