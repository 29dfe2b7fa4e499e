"""GPU tests of the flat store's writers (FlatWrite, api_entry_ctx_flat.inc.h) — run with -m gpu.
Every entry that changes a flat store orders its stream behind a mutation that is still only enqueued on another stream, whatever it
does afterwards: a store that grows is copied on the writer's stream, and a row overwritten in place is packed there.  The cases put
each writer directly behind an append_dev that waits on a caller's stream behind a few large matrix products, and then compare the
whole store, bit for bit, with a host model.  All rows are small integers: exact in fp16 and fp32, so a row's distance to itself is 0.
The last two tests are about the hole bits (HoleBits, api_types.inc.h): their device copy outgrown by bulk appends, and gaps that end
at the edges of their 64-bit words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2 = "SquaredEuclidean"
DIM = 48


@pytest.fixture(scope="module")
def zv():
    import zvec_amd
    return zvec_amd


@pytest.fixture(scope="module")
def side():
    """a caller's stream, and a matrix whose products keep it busy (one product up front: the library is loaded before a test needs it)"""
    import torch
    dev = torch.device("cuda", 0)
    a = torch.ones((4096, 4096), dtype=torch.float32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.mm(a, a)
    torch.cuda.synchronize()
    return s, a


def _busy(side):
    import torch
    s, a = side
    with torch.cuda.stream(s):
        for _ in range(6):
            torch.mm(a, a)
    return s.cuda_stream


def _still_busy(side):
    """the premise of a case: the append just enqueued on the caller's stream has not run yet"""
    return not side[0].query()


def _int_rows(rng, n, dtype):
    return rng.integers(-8, 9, (n, DIM)).astype(dtype)


def _blocks(rows, keys, bvc=32):
    """FlatStreamerEntity's persisted blocks: [bvc rows][bvc u64 keys][DeletionMap 4 B][BlockHeader 12 B], every row live"""
    n = rows.shape[0]
    rb = rows.shape[1] * rows.itemsize
    bs = bvc * rb + bvc * 8 + 16
    nb = (n + bvc - 1) // bvc
    blob = bytearray(nb * bs)
    keep = np.zeros(nb, np.uint32)
    for b in range(nb):
        r = rows[b * bvc:(b + 1) * bvc]
        kk = keys[b * bvc:(b + 1) * bvc].astype(np.uint64)
        o = b * bs
        blob[o:o + r.nbytes] = r.tobytes()
        blob[o + bvc * rb:o + bvc * rb + kk.nbytes] = kk.tobytes()
        keep[b] = (1 << len(r)) - 1 if len(r) < 32 else 0xffffffff
    return bytes(blob), nb, bs, keep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.itemsize == 2 else np.uint32)


WRITERS = ["append", "put_tail", "put_over", "load_features", "load_blocks", "reserve"]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("writer", WRITERS)
def test_writer_behind_a_pending_append_on_a_callers_stream_keeps_its_rows(zv, side, writer, dtype):
    import torch
    from zvec_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(WRITERS.index(writer) * 2 + (dtype == "fp16"))
    st = zv.HipFlatStreamer(DIM, L2, dtype=dtype)
    n0, n1, n2 = 300, 200, 1000
    first, pend, new = (_int_rows(rng, n, st.np_dtype) for n in (n0, n1, n2))
    assert st.add_batch(first) == 0
    # room for the pending rows, so that their append only enqueues (a growing store is copied and synchronised, which would drain
    # the caller's stream before the writer is called); the writer's rows, or its 8 * count, are past it: the store grows there
    assert st.reserve(640) == 0
    d = torch.from_numpy(pend).to("cuda:0")          # alive until the synchronise below
    torch.cuda.synchronize()
    stream = _busy(side)
    assert st.add_batch_dev(d.data_ptr(), n1, stream=stream) == 0
    assert _still_busy(side)
    model = np.concatenate([first, pend])
    n = n0 + n1
    tail = np.arange(n, n + n2)
    if writer == "append":
        assert st.add_batch(new) == 0
        model = np.concatenate([model, new])
    elif writer == "put_tail":
        assert st.add_with_id_batch(tail.astype(np.uint32), new) == 0
        model = np.concatenate([model, new])
    elif writer == "put_over":                       # 20 pending rows overwritten before the store grows, 20 after
        over = n0 + rng.choice(n1, 40, replace=False)
        ids = np.concatenate([over[:20], tail[:n2 - 40], over[20:]])
        assert st.add_with_id_batch(ids.astype(np.uint32), new) == 0
        model = np.concatenate([model, new[20:n2 - 20]])
        model[over[:20]] = new[:20]
        model[over[20:]] = new[n2 - 20:]
    elif writer == "load_features":
        keys = tail.astype(np.uint64)
        assert L.zvec_hip_flat_load_features(st._h, new.tobytes(), new.nbytes, n2, 0, 32, keys.ctypes.data) == 0
        model = np.concatenate([model, new])
    elif writer == "load_blocks":
        blob, nb, bs, keep = _blocks(new, tail)
        assert L.zvec_hip_flat_load_blocks(st._h, blob, len(blob), nb, bs, 32, keep.ctypes.data) == 0
        model = np.concatenate([model, new])
    else:
        assert st.reserve(8 * n) == 0
    torch.cuda.synchronize()
    del d
    assert st.count() == len(model)
    got = st.get_vectors_by_ids(np.arange(len(model)))
    bad = np.nonzero((_bits(got) != _bits(model)).any(1))[0]
    assert bad.size == 0, "%s/%s: %d rows differ from the host model, first at %s" % (writer, dtype, bad.size, bad[:8])
    # four of the rows that went in on the caller's stream (not overwritten, and met nowhere else) are their own nearest rows
    qpos = [p for p in range(n0, n) if np.array_equal(model[p], pend[p - n0]) and (model == model[p]).all(1).sum() == 1][::45][:4]
    assert len(qpos) == 4
    ctx = st.create_context()
    ctx.set_topk(5)
    assert st.search_impl(model[qpos], 4, ctx) == 0
    assert np.array_equal(ctx.counts, np.full(4, 5, np.uint32))
    assert np.array_equal(ctx.keys[:, 0], np.array(qpos, np.uint64))
    assert np.array_equal(ctx.scores[:, 0], np.zeros(4, np.float32))


def test_fp32_to_bits_append_behind_a_pending_one_on_a_callers_stream(zv, side):
    import torch
    from tests.binary_quant_ref import binary_encode_reference
    dim = 96
    rng = np.random.default_rng(9)
    a = rng.standard_normal((130, dim)).astype(np.float32)
    b = rng.standard_normal((600, dim)).astype(np.float32)
    se = zv.HipFlatStreamer(dim, "Hamming", dtype="binary32")
    d = torch.from_numpy(a).to("cuda:0")
    torch.cuda.synchronize()
    stream = _busy(side)
    assert se.add_batch_fp32_dev(d.data_ptr(), 130, dim, stream=stream) == 0
    assert _still_busy(side)
    assert se.add_batch_fp32(b) == 0
    torch.cuda.synchronize()
    del d
    want = binary_encode_reference(np.concatenate([a, b]))
    assert se.count() == 730
    assert np.array_equal(se.get_vectors_by_ids(np.arange(730)), want)


def test_single_row_adds_stay_ordered_across_holes_and_growth(zv):
    """64 one-row add_with_id calls through the pinned ring, appends alternating with overwrites in place; gaps of 1 and of 70
    positions cross a word of the hole bits (64 positions) and the store's first tile (128 rows: it grows inside the run)"""
    rng = np.random.default_rng(3)
    st = zv.HipFlatStreamer(DIM, L2)
    gaps = {8: 1, 16: 70, 40: 1, 48: 70}
    model, holes, n = {}, set(), 0
    for i in range(64):
        row = _int_rows(rng, 1, np.float32)[0]
        if i % 2 == 0:
            doc = n + gaps.get(i, 0)
            holes.update(range(n, doc))
            n = doc + 1
        elif i in (21, 53):                          # onto a hole
            doc = sorted(holes)[len(holes) // 2]
            holes.discard(doc)
        else:
            doc = int(rng.choice(sorted(model)))
        assert st.add_with_id_impl(doc, row) == 0
        model[doc] = row
    assert n > 128 and len(holes) == 140
    assert st.count() == n and st.holes() == len(holes)
    want = np.zeros((n, DIM), np.float32)
    for p, r in model.items():
        want[p] = r
    assert np.array_equal(_bits(st.get_vectors_by_ids(np.arange(n))), _bits(want))
    live = len(model)
    ctx = st.create_context()
    ctx.set_topk(live + 10)
    assert st.search_impl(want[sorted(model)[:2]], 2, ctx) == 0
    for qi in range(2):
        assert ctx.counts[qi] == live
        assert sorted(int(k) for k in ctx.keys[qi, :live]) == sorted(model)


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _copy_room(rows):
    """rows the device copy of the hole bits has room for after HoleBits::reserve(rows) made it: words_for(rows) = (rows + 63) // 64
    + 1 words are asked for as DevBuf::ensure(16 bytes a word), which allocates a quarter more and 256 bytes; one word stays spare"""
    words = (rows + 63) // 64 + 1
    return ((16 * words + 16 * words // 4 + 256) // 8 - 1) * 64


@pytest.mark.parametrize("kind", ["fp32", "binary64"])
def test_bulk_appends_to_a_handle_with_holes_across_growths_of_the_hole_copy(zv, kind):
    """One row at id 70 leaves 70 holes and a device copy of the hole bits made for 71 rows: 3 words, 316 bytes, 39 whole words, room
    for 2432 rows.  Appending 2500 rows (2571 > 2432) outgrows it: 42 words, 1096 bytes, 137 words, room for 8704 rows.  Appending
    6500 more (9071 > 8704) outgrows it again.  Every search reads the copy's words for all rows, so after each call no hole may
    come back, with and without a caller's exclude set.  Scores are exact integers on both handles (integer-valued fp32 rows at
    dim 32 against fp64; 64-bit rows under Hamming, which reads the exclude set through its own kernel): only ties are free."""
    from tests.hamming_ref import check_hamming_lists, hamming_reference
    rng = np.random.default_rng(70)
    bulks = (2500, 6500)
    assert 71 + bulks[0] > _copy_room(71) == 2432 and 71 + sum(bulks) > _copy_room(71 + bulks[0]) == 8704
    if kind == "fp32":
        st = zv.HipFlatStreamer(32, L2)
        make = lambda n: rng.integers(-8, 9, (n, 32)).astype(np.float32)
        score = lambda b, q: ((b.astype(np.float64)[None] - q.astype(np.float64)[:, None]) ** 2).sum(-1).astype(np.int64)
    else:
        st = zv.HipFlatStreamer(64, "Hamming", dtype="binary64")
        make = lambda n: rng.integers(0, 2**64, (n, 1), dtype=np.uint64)
        score = hamming_reference
    q = make(3)
    q[2] = 0                                         # (nearest to the holes' zero rows)
    stored = np.zeros((71, q.shape[1]), q.dtype)
    stored[70] = make(1)[0]
    assert st.add_with_id_impl(70, stored[70]) == 0
    for step, n_new in enumerate((0,) + bulks):
        if n_new:
            new = make(n_new)
            assert st.add_batch(new) == 0
            stored = np.concatenate([stored, new])
        n = stored.shape[0]
        assert st.count() == n and st.holes() == 70
        ref = score(stored, q)
        live = np.arange(n) >= 70
        # the caller's set: every 7th position, and each query's best live row
        ex = np.arange(n) % 7 == 3
        ex[[70 + int(np.argmin(ref[i, 70:])) for i in range(3)]] = True
        for mask in (None, ex):
            ctx = st.create_context()
            ctx.set_topk(10)
            if mask is not None:
                ctx.set_exclude_bitset(_words_of(mask))
            assert st.search_impl(q, 3, ctx) == 0
            assert (ctx.keys[:, :10][ctx.counts[:, None] > np.arange(10)[None]] >= 70).all(), "step %d: a hole came back" % step
            check_hamming_lists(ctx.keys, ctx.scores, ctx.counts, ref, 10, admissible=live if mask is None else live & ~mask,
                                what="%s step %d %s" % (kind, step, "plain" if mask is None else "exclude"))


@pytest.mark.parametrize("staged", [False, True])
def test_put_gaps_at_the_edges_of_the_hole_words(zv, staged):
    """Gaps [count, id) that end at positions 63, 65 and 128 on one handle and at 64 and 129 on another (a gap can end at 64 only where
    none ended at 63), then one of more than two words, then rows put onto positions 0, 63 and 64, which are holes on one handle or
    the other.  staged: the id is named ten times, which takes the put off the pinned ring (more than 8 rows) and overwrites the new
    row nine times.  After each put the hole count is the model's and a search for every row returns exactly the live positions."""
    rng = np.random.default_rng(63)
    for ids in ([63, 65, 128, 400, 0, 63, 64], [64, 129, 300, 0, 63, 64]):
        st = zv.HipFlatStreamer(32, L2)
        live, n = set(), 0
        for doc in ids:
            rows = rng.integers(-8, 9, (10 if staged else 1, 32)).astype(np.float32)
            assert st.add_with_id_batch(np.full(rows.shape[0], doc, np.uint32), rows) == 0
            live.add(doc)
            n = max(n, doc + 1)
            assert st.count() == n and st.holes() == n - len(live), "ids %r, after %d" % (ids, doc)
            ctx = st.create_context()
            ctx.set_topk(n)
            assert st.search_impl(rows[-1:], 1, ctx) == 0
            assert ctx.counts[0] == len(live)
            assert sorted(int(k) for k in ctx.keys[0, :len(live)]) == sorted(live), "ids %r, after %d" % (ids, doc)
            assert ctx.keys[0, 0] == doc and ctx.scores[0, 0] == 0          # (the last row named is the one stored)
