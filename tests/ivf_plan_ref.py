"""The IVF probe plan and the list scan's work items restated in plain integers and fp64, and the fixtures that push every loop of
the plan past its first pass (numpy only; nothing here touches the GPU or the library).

What is restated (zvec_amd/csrc/zvk_plan.hip.h, the item decode at the top of the list scan in zvk_scan.hip.h, the host sizing in
api_ivf_core.inc.h, the deal order and levels of host/ivf_layout.h):

  probe rule     a rank is probed while the rows of the lists BEFORE it stay below max_scan_count; plan_wave_kernel and
                 ivf_expand_direct_kernel evaluate it 64 ranks per pass with carries (scanned_before / before_g, slot_carry / before_l)
  slots          a probed, non-empty list gives the query one result slot per chunk of the list, numbered in probe order
  list-major CSR per list the (query, first slot) pairs of the queries probing it; the order inside a list comes from an atomicAdd
                 and is not defined, so it is held as a set
  exclusive scans slot_begin over queries, list_qoff over lists, item_off over the lists in deal order (plan_scan_kernel: blockDim.x
                 elements per round with a carry; 1024 threads on the context's own stream, 256 on a caller's)
  work items     item -> (list, chunk, group of 32 query rows): within / ngroups, within % ngroups
  answer         every query's top-k in the reference's order: score, then probe rank, then place in the list

Every restated loop takes a `drop` argument that forgets one carry (DROPS): the CPU test shows for every fixture that the answer
changes under it — that is how "the GPU test would fail" is shown without touching a kernel.

Fixtures: centroids on a line, centroid l at x = 2 l, a query at x = 2 j + 0.5: its distances to the centroids are |2 (j - l) + 0.5|,
all different, so the coarse ranking is untied over ALL lists and exact in fp32 and fp16.  Rows are small integers: every score is
exact in either format and compared bit for bit."""
import numpy as np

TILE = 128                      # rows of a store tile (IVF_TILE_ROWS)
ROWS_PER_GROUP = 32             # query rows of one work item
PASS = 64                       # probe ranks per pass of the wave kernels
HEAD_PCT = 50                   # share of the tiles dealt in double-length chunks (the library's default)
FUSED_MAX_K = 472               # the largest k whose lists fit in the scan's LDS: (162816 / 4 - 10468) / 64
DIRECT_MAX_Q = 8                # batches up to this many queries take the direct route (the library's default)
PKEYS_TOPK_MAX, RUN = 64, 1024
ROUTE_NONE, ROUTE_DIRECT_BLOCK_TOPK, ROUTE_DIRECT_SELECT, ROUTE_TILE, ROUTE_LARGE_K = 0, 1, 2, 3, 4
DROPS = ("scanned_before", "slot_carry", "scan_carry")


def tiles(size):
    return (np.asarray(size, np.int64) + TILE - 1) // TILE


# ---- host/ivf_layout.h: deal order and levels ------------------------------------------------------------------------------------------
def list_order(sizes):
    """lists by stored size, largest first (stable)"""
    return np.argsort(-np.asarray(sizes, np.int64), kind="stable")


def list_levels(sizes, head_pct=HEAD_PCT):
    """IvfLayout::finish: 2 for the lists at the end of the deal order that hold the last quarter of the tiles, 0 for those at its
    head that hold the first head_pct per cent, 1 in between"""
    sizes = np.asarray(sizes, np.int64)
    order, t = list_order(sizes), tiles(sizes)
    total = int(t.sum())
    level = np.ones(sizes.size, np.int64)
    acc = 0
    for l in order[::-1]:
        if acc * 4 >= total:
            break
        level[l] = 2
        acc += int(t[l])
    acc = 0
    for l in order:
        if acc * 100 >= total * head_pct or level[l] == 2:
            break
        level[l] = 0
        acc += int(t[l])
    return level


def level_tpc(level, tpc):
    """tiles per chunk of a list by its level: twice the search's base length (at most 32), the base length, a quarter (at least 1)"""
    level = np.asarray(level, np.int64)
    return np.where(level == 0, min(2 * tpc, 32), np.where(level == 1, tpc, max(1, tpc >> 2))).astype(np.int64)


def chunks_of(sizes, ltpc):
    t = tiles(sizes)
    return (t + ltpc - 1) // ltpc


def slots_bound(sizes, ltpc, nprobe, count):
    """api_ivf_core.inc.h: the slots one query can be dealt at most — the nprobe lists with the most chunks — times the batch"""
    ch = np.sort(np.where(np.asarray(sizes) > 0, chunks_of(sizes, ltpc), 0))[::-1]
    return max(1, int(ch[:nprobe].sum()) * int(count))


# ---- coarse ranking --------------------------------------------------------------------------------------------------------------------
def coarse_ranking(cent, queries, nprobe):
    """[nq][nprobe] list ids by squared distance in fp64 (ties by id) and the sorted distances of ALL lists"""
    d = ((queries.astype(np.float64)[:, None, :] - cent.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")
    return order[:, :nprobe], np.take_along_axis(d, order, 1)


# ---- zvk_plan.hip.h --------------------------------------------------------------------------------------------------------------------
def probe_rule(ranks, sizes, max_scan, brute_force=False, drop=None):
    """plan_wave_kernel / ivf_expand_direct_kernel, one query: the probed prefix of `ranks` in passes of 64 with the carry
    scanned_before (before_g).  Returns (probed ranks, rows scanned)."""
    n, before, scanned, probed = len(ranks), 0, 0, []
    for r0 in range(0, n, PASS):
        part = ranks[r0:r0 + PASS]
        sz = sizes[part]
        if drop == "scanned_before":
            before = 0
        excl = before + np.cumsum(sz) - sz
        ok = np.ones(len(part), bool) if brute_force else excl < max_scan
        probed += [int(l) for l in part[ok]]
        scanned += int(sz[ok].sum())
        before += int(sz.sum())
        if not brute_force and before >= max_scan:
            break
    return probed, scanned


def block_scan(v, nt, drop=None):
    """plan_scan_kernel's exclusive scan: nt elements per round, the running total carried into the next round"""
    v = np.asarray(v, np.int64)
    out, carry = np.zeros(v.size + 1, np.int64), 0
    for base in range(0, v.size, nt):
        part = v[base:base + nt]
        if drop == "scan_carry":
            carry = 0
        out[base:base + part.size] = carry + np.cumsum(part) - part
        carry += int(part.sum())
    out[v.size] = carry
    return out


def plan(probe_lists, sizes, max_scan, ltpc, nt=1024, rows_per_group=ROWS_PER_GROUP, brute_force=False, drop=None):
    """Everything the plan kernels leave behind.  probe_lists: [nq][nprobe] list ids in coarse order (ignored under brute force:
    every list in id order); ltpc: tiles per chunk of every list; nt: threads of plan_scan_kernel."""
    sizes = np.asarray(sizes, np.int64)
    nlist = sizes.size
    nq = len(probe_lists)
    ch = np.where(sizes > 0, chunks_of(sizes, ltpc), 0)
    probed, q_nprobe, q_scanned, q_nslots, local = [], np.zeros(nq, np.int64), np.zeros(nq, np.int64), np.zeros(nq, np.int64), []
    list_count = np.zeros(nlist, np.int64)
    for q in range(nq):
        ranks = np.arange(nlist) if brute_force else np.asarray(probe_lists[q], np.int64)
        pr, sc = probe_rule(ranks, sizes, max_scan, brute_force, drop)
        probed.append(pr)
        q_nprobe[q], q_scanned[q] = len(pr), sc
        # slot of every probed non-empty list, relative to the query's first slot: the chunks of the lists before it, with the
        # carry slot_carry between passes of 64 RANKS (probed ranks are a prefix, so ranks and places in `pr` coincide)
        carry, rel = 0, []
        for r0 in range(0, len(pr), PASS):
            part = np.asarray(pr[r0:r0 + PASS], np.int64)
            c = ch[part]
            if drop == "slot_carry":
                carry = 0
            rel += list(carry + np.cumsum(c) - c)
            carry += int(c.sum())
        q_nslots[q] = carry
        local.append(rel)
        for l in pr:
            if sizes[l]:
                list_count[l] += 1
    slot_begin = block_scan(q_nslots, nt, drop)
    list_qoff = block_scan(list_count, nt, drop)
    order = list_order(sizes)
    items = (list_count[order] + rows_per_group - 1) // rows_per_group * ch[order]
    item_off = block_scan(items, nt, drop)
    csr = [set() for _ in range(nlist)]
    for q in range(nq):
        for l, s in zip(probed[q], local[q]):
            if sizes[l]:
                csr[l].add((q, int(slot_begin[q] + s)))
    return dict(probed=probed, q_nprobe=q_nprobe, q_scanned=q_scanned, q_nslots=q_nslots, slot_begin=slot_begin, list_count=list_count,
                list_qoff=list_qoff, item_off=item_off, total_items=int(item_off[nlist]), csr=csr, order=order, chunks=ch,
                list_tpc=np.asarray(ltpc, np.int64), rows_per_group=rows_per_group)


# ---- answers ---------------------------------------------------------------------------------------------------------------------------
def list_offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def scores_of(rows, query):
    return ((rows.astype(np.float64) - query.astype(np.float64)[None, :]) ** 2).sum(1)


def topk_reference(probed, sizes, vecs, queries, k, excluded=None):
    """every query's k best rows of its probed lists in the reference's order: score, then probe rank, then place in the list.
    Returns positions [nq][k] (list-order positions, -1 beyond the count), fp64 scores, counts."""
    offs = list_offsets(sizes)
    nq = len(probed)
    pos, sc, cnt = np.full((nq, k), -1, np.int64), np.zeros((nq, k)), np.zeros(nq, np.int64)
    for q in range(nq):
        cand = np.concatenate([np.arange(offs[l], offs[l + 1]) for l in probed[q]] + [np.zeros(0, np.int64)]).astype(np.int64)
        if excluded is not None:
            cand = cand[~excluded[cand]]
        s = scores_of(vecs[cand], queries[q])
        best = np.argsort(s, kind="stable")[:k]
        cnt[q] = best.size
        pos[q, :best.size], sc[q, :best.size] = cand[best], s[best]
    return pos, sc, cnt


def simulate_scan(pl, sizes, vecs, queries, k, excluded=None, swap_decode=False):
    """The list scan and its merge driven by a plan `pl` AS THE KERNEL DECODES IT: item -> list by item_off, chunk = within / ngroups,
    group = within % ngroups, the rows of the group from the CSR, slot = csr_slot + chunk; every (row, item) leaves its k best rows
    of the chunk's tiles in its slot, a query's answer is merged from slots [slot_begin[q], slot_begin[q + 1]).  A slot written twice
    keeps the last writer, a slot never written holds nothing — which is how a wrong plan shows.  swap_decode: chunk and group
    exchanged.  Returns (positions, scores, counts) like topk_reference (order: score, slot, place)."""
    sizes = np.asarray(sizes, np.int64)
    offs, nlist, rpg = list_offsets(sizes), sizes.size, pl["rows_per_group"]
    csr_q, csr_slot = np.zeros(int(pl["list_qoff"][nlist]) + 1, np.int64), np.zeros(int(pl["list_qoff"][nlist]) + 1, np.int64)
    for l in range(nlist):
        for j, (q, s) in enumerate(sorted(pl["csr"][l])):
            e = int(pl["list_qoff"][l]) + j
            if e < csr_q.size:
                csr_q[e], csr_slot[e] = q, s
    slots = {}
    item_off = pl["item_off"]
    for item in range(pl["total_items"]):
        lo = int(np.searchsorted(item_off[:nlist], item, side="right")) - 1
        li = int(pl["order"][lo])
        within = item - int(item_off[lo])
        qcnt = int(pl["list_qoff"][li + 1] - pl["list_qoff"][li])
        ngroups = (qcnt + rpg - 1) // rpg
        if ngroups == 0:
            continue
        chunk, group = within // ngroups, within % ngroups
        if swap_decode:
            chunk, group = within % ngroups, within // ngroups
        tpc = int(pl["list_tpc"][li])
        r_lo, r_hi = min(chunk * tpc * TILE, int(sizes[li])), min((chunk + 1) * tpc * TILE, int(sizes[li]))
        rows = np.arange(offs[li] + r_lo, offs[li] + r_hi)
        if excluded is not None:
            rows = rows[~excluded[rows]]
        for j in range(group * rpg, min(group * rpg + rpg, qcnt)):
            e = int(pl["list_qoff"][li]) + j
            if e >= csr_q.size:                 # (a wrong plan reads past the CSR: nothing usable there)
                continue
            q = int(csr_q[e])
            s = scores_of(vecs[rows], queries[q])
            best = np.argsort(s, kind="stable")[:k]
            slots[int(csr_slot[e]) + chunk] = (rows[best], s[best])
    nq = len(queries)
    pos, sc, cnt = np.full((nq, k), -1, np.int64), np.zeros((nq, k)), np.zeros(nq, np.int64)
    for q in range(nq):
        got = [slots[s] for s in range(int(pl["slot_begin"][q]), int(pl["slot_begin"][q + 1])) if s in slots]
        if not got:
            continue
        r, s = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        best = np.argsort(s, kind="stable")[:k]
        cnt[q] = best.size
        pos[q, :best.size], sc[q, :best.size] = r[best], s[best]
    return pos, sc, cnt


def same_answer(a, b):
    """equal counts and equal score lists (the rows may differ among equal scores)"""
    return np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1])


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
def line_centroids(nlist, dim):
    c = np.zeros((nlist, dim), np.float32)
    c[:, 0] = 2.0 * np.arange(nlist)
    return c


def line_queries(js, dim, rng, gaussian=False):
    """a query per j: x = 2 j + 0.5 on the centroids' line, small integers (or gaussian values) elsewhere — every query differs"""
    js = np.asarray(js, np.int64)
    q = rng.standard_normal((js.size, dim)).astype(np.float32) if gaussian else rng.integers(0, 16, (js.size, dim)).astype(np.float32)
    q[:, 0] = 2.0 * js + 0.5
    return q


def rows_for(sizes, dim, rng, gaussian=False):
    n = int(np.sum(sizes))
    return rng.standard_normal((n, dim)).astype(np.float32) if gaussian else rng.integers(0, 16, (n, dim)).astype(np.float32)


def keys_for(n):
    """keys that are neither positions nor dense: a returned position cannot pass for a key"""
    return (np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1000003))


def exclusion(n, seed=5):
    """about 30 % of the list-order positions excluded"""
    return np.random.default_rng(seed).random(n) < 0.3


def pack_bits(mask):
    words = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return words


P_RANKS_NLIST, P_RANKS_ROWS = 200, 30
# (nprobe, max_scan_count) -> lists probed with 30 rows per list: the rule admits rank r while 30 r < max_scan_count
P_RANKS_PAIRS = ((150, 1920), (150, 1921), (150, 3840), (150, 3841), (200, 6000))
P_RANKS_PROBED = {(150, 1920): 64, (150, 1921): 65, (150, 3840): 128, (150, 3841): 129, (200, 6000): 200}


def p_ranks(sizes="equal", nq=40, dim=8, gaussian=False, seed=11):
    """200 lists; `equal`: 30 rows each, so the probe count does not depend on the ranking and the pass boundaries are exact;
    `unequal`: 1 ... 59 rows, so the cut falls at another rank in every query.  Queries spread over the whole line."""
    rng = np.random.default_rng(seed)
    nlist = P_RANKS_NLIST
    sz = np.full(nlist, P_RANKS_ROWS, np.int64) if sizes == "equal" else 1 + (np.arange(nlist) * 37) % 59
    js = (np.arange(nq) * (nlist - 1)) // max(nq - 1, 1)
    return dict(name="p_ranks_" + sizes, nlist=nlist, dim=dim, sizes=sz, cent=line_centroids(nlist, dim),
                queries=line_queries(js, dim, rng, gaussian), vecs=rows_for(sz, dim, rng, gaussian), gaussian=gaussian)


P_ROUNDS_NLIST, P_ROUNDS_NQ, P_ROUNDS_NPROBE = 1064, 1061, 3
P_ROUNDS_UNPROBED = (0, 255, 256, 1023, 1024, 1063)      # no query comes within three ranks of them
P_ROUNDS_EMPTY = (1062, 1063)                            # no rows (1062 is probed all the same)


def p_rounds(dim=8, seed=12):
    """1064 lists of 3 ... 9 rows, sizes falling with the list id, so the deal order IS the id order and a list's place in item_off
    is its id; 1061 queries probing 3 lists each.  Both scans of plan_scan_kernel over queries and lists take two rounds with 1024
    threads and five with 256, with runs of zero-item lists across elements 255 | 256 and 1023 | 1024 and at both ends."""
    rng = np.random.default_rng(seed)
    nlist = P_ROUNDS_NLIST
    sz = 9 - (np.arange(nlist) * 7) // nlist
    sz[list(P_ROUNDS_EMPTY)] = 0
    # query j probes lists j, j + 1, j - 1: keep every j away from the unprobed lists
    banned = {u + d for u in P_ROUNDS_UNPROBED for d in (-1, 0, 1)}
    js = [j for j in range(1, nlist - 2) if j not in banned]
    js = np.asarray((js + js)[:P_ROUNDS_NQ], np.int64)
    return dict(name="p_rounds", nlist=nlist, dim=dim, sizes=sz, cent=line_centroids(nlist, dim), queries=line_queries(js, dim, rng),
                vecs=rows_for(sz, dim, rng), gaussian=False)


P_GROUPS_SIZES = (9 * TILE + 1, 1, 128, 500, 127, 129)   # levels 0, 2, 2, 1, 2, 2 (test_ivf_plan_reference_cpu.py)
P_GROUPS_BATCHES = (16, 17, 32, 33, 48, 49, 65, 97)      # last group of 16, 17, 32, 1, 16, 17, 1, 1 rows


def p_groups(nq, dim=16, seed=13):
    """six lists, every query nearest to list 0 and probing all six: every list is probed by the whole batch, so its rows are dealt
    in groups of 32 with a last group of nq % 32 rows.  Sizes of 1, 127, 128, 129, 500 and nine tiles plus one row put lists on all
    three chunk levels (the issue's "4 lists" cannot hold its five sizes AND a middle level: six can)."""
    sz = np.asarray(P_GROUPS_SIZES, np.int64)
    js = -(np.arange(nq) % 8)
    # (the rows from a generator of their own: they are the same for every batch size, one index serves all)
    return dict(name="p_groups_%d" % nq, nlist=sz.size, dim=dim, sizes=sz, cent=line_centroids(sz.size, dim),
                queries=line_queries(js, dim, np.random.default_rng(seed + 1)), vecs=rows_for(sz, dim, np.random.default_rng(seed)),
                gaussian=False)


def group_shapes(nq, rows_per_group=ROWS_PER_GROUP):
    """(groups, rows of the last group) of a list probed by nq queries"""
    g = (nq + rows_per_group - 1) // rows_per_group
    return g, nq - (g - 1) * rows_per_group


def expected_route(nq, k, nprobe, sizes, brute_force=False):
    """the route ivf_search_core dispatches for these fixtures (api_ivf_core.inc.h; rows and bytes are far below its other limits)"""
    if not brute_force and nq <= DIRECT_MAX_Q:
        rows = int(np.sort(np.asarray(sizes, np.int64))[::-1][:nprobe].sum())
        stride = (max(rows, 1) + 63) // 64 * 64
        return ROUTE_DIRECT_BLOCK_TOPK if stride > RUN and k <= PKEYS_TOPK_MAX else ROUTE_DIRECT_SELECT
    return ROUTE_LARGE_K if k > FUSED_MAX_K else ROUTE_TILE
