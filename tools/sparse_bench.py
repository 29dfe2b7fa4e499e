"""Flat sparse inner-product search, 1M rows of 64-192 elements over a 30 522-word vocabulary with Zipf-distributed indices, queries
of 16-64 elements, k = 10, batches 1 / 64 / 1024: QPS and ms per step against two bounds of the box it runs on (reported, not
gated; bench.py is the project's benchmark and does not cover sparse rows).

  streaming bound  stored bytes of the index (8 per element + 16 per row; 6 per element with --dtype fp16) / the box's streaming
                   figure (zvec_hip_calibrate, same process): batch 1
  LDS-issue bound  every stored element costs every query block ceil(log2(longest run of the block)) + 1 probes of the block's
                   LDS image; a probe is one ds_read_b32 wave instruction = 2 LDS cycles when conflict-free, one LDS per CU:
                   elements x blocks x probes x 2 / (CUs x calibrated clock).  Lanes probe unrelated addresses, so bank
                   conflicts come on top: the bound is not reachable, the fraction says how far the scan is from it.

    python tools/sparse_bench.py [--dtype fp32|fp16] [--out profiles/sparse_flat1m.json] [--steps 10] [--warmup 3]

--dtype fp16: the same corpus and the same queries with every value rounded to half, in an index of fp16 values
(zvec_hip_sparse_create_typed(ZVEC_HIP_DT_FP16, ...)); the LDS-issue bound is unchanged (a half is still one probe).

--by-keys: the same corpus searched by primary keys (zvec_hip_sparse_search_by_ids): 100 / 10 000 / 100 000 random distinct rows
listed per query, batches 1 / 64, host-pointer call to host-pointer call (wall clock, median of the steps, the upload of the lists
included).  Next to it the only other route to the same answer: zvec_hip_sparse_search with an exclude bitset set on every row
that is not listed, which takes ONE bitset per call, so a batch whose queries have lists of their own is one call per query
(bitsets made before the clock starts).  Both in one process, answers compared.

  gather bound  8 bytes (fp16: 6) per listed element + 16 per listed row / the box's streaming figure (zvec_hip_calibrate, same
                process)

    python tools/sparse_bench.py --by-keys [--out profiles/sparse_by_keys.json] [--steps 10] [--warmup 3]

--grouped: the same corpus under group-by search (zvec_hip_sparse_search_grouped): 1000 groups dealt at random, group_num 10 x
group_topk 10, batches 1 / 2 / 4 / 8 / 16 / 32 / 64, host-pointer call to return (wall clock, median of the steps).  Every batch
is timed with "sparse_group_rows" at 0 (the lane = query score dump) and at 64 (the wave-per-row score dump), and next to them the
plain zvec_hip_sparse_search (k = 10) of the same queries; the answers of the two dumps are compared.  The default of
"sparse_group_rows" is read off this file: the largest batch up to which the wave-per-row dump was the faster one.

    python tools/sparse_bench.py --grouped [--dtype fp32|fp16] [--out profiles/sparse_grouped.json] [--steps 10] [--warmup 3]

--metric l2: the chosen mode runs twice in one process, on an InnerProductSparse index and then on a SquaredEuclideanSparse index
(zvec_hip_sparse_create_metric(.., ZVEC_HIP_METRIC_L2, ..)) of the same corpus with the same queries; every figure of the L2 run
is reported beside the IP figure of the same point under an "l2_" name (reported, not gated).  The L2 scan does strictly more
work per stored element (a square for every element, two more sums on a hit) and has no shortcut for an empty query.

    python tools/sparse_bench.py --metric l2 [--by-keys | --grouped] [--dtype fp32|fp16] [--out profiles/sparse_flat1m_l2.json]

--inverted: the full-scan mode's corpus and queries (batches 1 / 64 / 1024, k = 10, device-pointer call on a stream, device events)
searched twice in one process, by the row scan and through the term-major twin (zvec_hip_sparse_set_inverted), for fp32 and for fp16
values: ms per step of both routes, the twin's build time (the first search after it was asked for, wall clock, minus a later step),
its bytes and term count, and whether the two answers agree (every list full and ascending, scores within agreement_band of each
other place by place).  Reported, not gated; InnerProductSparse only.

It then times ONE build of the twin on each route of the option "sparse_inverted_build" (0 = host, 1 = device: zvk_sparse_invb.hip.h)
on the same handle: the lists are dropped and asked for again (set_inverted(0) / set_inverted(1)), one search forces the build, and
zvec_hip_sparse_inverted_build_info tells its route, digit passes and wall-clock ms.  These go to --build-out with the box's
streaming figure (zvec_hip_calibrate, same process) and the bytes the device build cannot avoid moving over that figure as its bound:

  build bytes   per element: 4 read for the OR; per digit pass 4 read for the histogram, 4 (first pass: the indices) or 8 (key and
                ordinal) read and 8 written for the scatter; 4 written for the positions; 2 x 4 read for the heads; 4 + 4 + value
                read and 4 + value written for the postings; per row 8 read (row offsets); per term 12 written.  The count
                tables are left out (1 / 2 byte per element and pass), and so is every miss of the scatter's and the gathers' lines.

    python tools/sparse_bench.py --inverted [--out profiles/sparse_inverted.json] [--build-out profiles/sparse_inverted_build.json]
                                 [--steps 10] [--warmup 3]

    --put       add-with-id (zvec_hip_sparse_put) on the full-scan mode's corpus, one call on each route: 0 tail (--put-rows new rows
                behind the last one), 1 in place (as many random rows replaced by rows of their own length), 2 splice (the same rows
                replaced by rows one element longer or shorter, so that everything behind the first of them moves).  Reported per
                route: the call's wall clock (zvec_hip_sparse_put_info), the pairs the device wrote and the bytes per second they
                make (4 + value bytes a pair, read and written: twice that), next to the box's calibrated streaming rate.  One call
                each, not repeated; reported, not gated.

    python tools/sparse_bench.py --put [--dtype fp32|fp16] [--put-rows 1000] [--out profiles/sparse_put.json]

    --put --from-device   the same three calls with the call's rows already in device memory (zvec_hip_sparse_put_dev), next to the
                host zvec_hip_sparse_put of the same rows on a second handle that holds the same corpus, in the same process.
                Reported per route: ms per call of either entry (zvec_hip_sparse_put_info), the moved bytes per second, and the
                box's calibrated streaming rate.  One call each, not repeated; reported, not gated.

    python tools/sparse_bench.py --put --from-device [--dtype fp32|fp16] [--put-rows 1000] [--out profiles/sparse_put_dev.json]

    --ingest    rows and queries that are dense matrices in device memory, what a learned sparse encoder leaves there
                (zvec_hip_sparse_append_dense_dev, zvec_hip_sparse_search_dense_dev).  The full-scan mode's corpus is scattered into
                dense rows over the vocabulary on the device, --ingest-rows rows at a time (the whole matrix does not fit), and every
                block is appended as it stands.  Reported: the appends' wall clock (zvec_hip_sparse_ingest_info) and the bytes of
                the matrix they read per second (the matrix is read twice: count, then fill), one dense search at batches 1, 64
                and 1024 (device events around the steps), and, on the first --ingest-host-blocks blocks, the host route on the same
                data: copy the block to the host, numpy nonzero, zvec_hip_sparse_append.  All next to the box's calibrated
                streaming rate.  Reported, not gated.

    python tools/sparse_bench.py --ingest [--dtype fp32|fp16] [--ingest-rows 8192] [--out profiles/sparse_ingest.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


METRIC_NAMES = {"ip": "InnerProductSparse", "l2": "SquaredEuclideanSparse"}


def agreement_band(metric):
    """how far two routes to the same score may lie apart on this corpus (values below 1, rows of at most 192 and queries of at
    most 64 elements): twice the distance of either from the exact score.  ip: an fp32 sum of m <= 64 products,
    (m + 1) * 2^-23 * sum |products| <= 65 * 2^-23 * 64.  l2 (include/zvec_hip.h, Score): (rlen + 4) * 2^-23 * A + (qlen + 4) *
    2^-23 * (Qn + Mq) with A <= 192 * 4 and Qn, Mq <= 64"""
    if metric == "l2":
        return 2 * (196 * 2.0 ** -23 * 768 + 68 * 2.0 ** -23 * 128)
    return 2 * 65 * 2.0 ** -23 * 64


def beside(ip, l2, rows):
    """the L2 run's figures into the IP run's result: every entry of l2[rows] that differs goes beside its IP figure as "l2_" + name"""
    assert len(ip[rows]) == len(l2[rows])
    for a, b in zip(ip[rows], l2[rows]):
        a.update({"l2_" + key: value for key, value in b.items() if a.get(key) != value})
    ip.update({"l2_" + key: value for key, value in l2.items() if key != rows and ip.get(key) != value})
    ip["metric"] = "ip, l2 beside it"
    return ip


def zipf_runs(torch, dev, g, n, lo, hi, vocab, draws):
    """n runs of lo..hi distinct Zipf(1)-distributed indices, ascending: counts (int64 cpu), indices (int32 cpu)"""
    cdf = torch.cumsum(1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64), 0)
    cdf = (cdf / cdf[-1]).to(torch.float32)
    counts, parts = [], []
    for a in range(0, n, 50000):
        m = min(50000, n - a)
        w = torch.searchsorted(cdf, torch.rand((m, draws), generator=g, device=dev)).clamp_(max=vocab - 1)
        w, _ = torch.sort(w, dim=1)
        dup = torch.zeros_like(w, dtype=torch.bool)
        dup[:, 1:] = w[:, 1:] == w[:, :-1]
        # a random subset of the distinct words of the run: the `want` smallest random priorities among them
        pri = torch.rand((m, draws), generator=g, device=dev)
        pri[dup] = 2.0
        want = torch.randint(lo, hi + 1, (m,), generator=g, device=dev)
        want = torch.minimum(want, (~dup).sum(1))
        rank = torch.argsort(torch.argsort(pri, dim=1), dim=1)
        keep = rank < want[:, None]
        counts.append(want.cpu())
        parts.append(w[keep].to(torch.int32).cpu())          # (row-major: ascending inside a run)
    return torch.cat(counts), torch.cat(parts)


def by_keys(args, metric):
    import time
    import numpy as np
    import torch
    import zvec_amd
    from zvec_amd.index import _np_ptr
    L = zvec_amd._lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    rv = (torch.rand(ri.numel(), generator=g, device=dev) * 2 - 1).cpu()
    row_len = rc_.numpy().astype(np.int64)
    np_val = np.float16 if args.dtype == "fp16" else np.float32
    elem_bytes = 4 + np.dtype(np_val).itemsize
    se = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    assert se.reserve(args.n, ri.numel()) == 0
    assert se.add_batch(row_len.astype(np.uint32), ri.numpy().view(np.uint32), rv.numpy().astype(np_val)) == 0
    del ri, rv
    ctx = se.create_context()
    rng = np.random.default_rng(1)
    k = args.topk
    fmax = float(np.finfo(np.float32).max)

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), float(min(t))

    points = []
    for batch in (1, 64):
        qc, qi = zipf_runs(torch, dev, g, batch, 16, 64, args.vocab, 256)
        qv = (torch.rand(qi.numel(), generator=g, device=dev) * 2 - 1).cpu().numpy().astype(np_val)
        qc = qc.numpy().astype(np.uint32)
        qi = qi.numpy().view(np.uint32).copy()
        qo = np.zeros(batch + 1, np.int64)
        np.cumsum(qc, out=qo[1:])
        for length in (100, 10_000, 100_000):
            if length > args.n:
                continue
            lists = [rng.choice(args.n, length, replace=False).astype(np.uint32) for _ in range(batch)]
            ids = np.concatenate(lists)
            offs = (np.arange(batch + 1, dtype=np.uint64) * length).astype(np.uint32)
            keys = np.zeros((batch, k), np.uint64)
            scores = np.zeros((batch, k), np.float32)
            counts = np.zeros(batch, np.uint32)

            def new_entry():
                rc = L.zvec_hip_sparse_search_by_ids(se._h, ctx._h, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), batch, _np_ptr(ids), _np_ptr(offs),
                                                     k, fmax, None, _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
                assert rc == 0, rc
            new_ms, new_min = median_ms(new_entry)
            # the other route: every bit set except the listed rows', one call per query
            words = (args.n + 63) // 64
            bitsets = np.full((batch, words), 0xffffffffffffffff, np.uint64)
            for q in range(batch):
                np.bitwise_and.at(bitsets[q], lists[q] // 64, ~(np.uint64(1) << (lists[q] % 64).astype(np.uint64)))
            keys2 = np.zeros((batch, k), np.uint64)
            scores2 = np.zeros((batch, k), np.float32)
            counts2 = np.zeros(batch, np.uint32)

            def bitset_route():
                for q in range(batch):
                    rc = L.zvec_hip_sparse_search(se._h, ctx._h, _np_ptr(qc[q:q + 1]), _np_ptr(qi[qo[q]:qo[q + 1]]), _np_ptr(qv[qo[q]:qo[q + 1]]),
                                                  1, k, fmax, _np_ptr(bitsets[q]), _np_ptr(keys2[q:q + 1]), _np_ptr(scores2[q:q + 1]),
                                                  _np_ptr(counts2[q:q + 1]))
                    assert rc == 0, rc
            old_ms, old_min = median_ms(bitset_route)
            # the same answer up to the order of the sums (agreement_band: the k-th candidates may swap inside that band, their
            # scores stay within it)
            assert counts.tolist() == counts2.tolist() == [k] * batch
            assert bool(np.all(scores[:, 1:] >= scores[:, :-1])) and float(np.abs(scores - scores2).max()) <= agreement_band(metric)
            elements = int(sum(int(row_len[a].sum()) for a in lists))
            points.append({"batch": batch, "keys_per_query": length, "by_ids_ms": new_ms, "by_ids_min_ms": new_min, "bitset_route_ms": old_ms,
                           "bitset_route_min_ms": old_min, "speedup": old_ms / new_ms, "listed_elements": elements,
                           "gathered_bytes": elements * elem_bytes + batch * length * 16})
            print(json.dumps(points[-1]), flush=True)
    del se
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = L.zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for p in points:
        p["gather_bound_ms"] = p["gathered_bytes"] / (gbs.value * 1e9) * 1e3
        p["bound_fraction"] = p["gather_bound_ms"] / p["by_ids_ms"]
    res = {"workload": "flat sparse %s %d rows x 64-192 of %d (Zipf), queries 16-64, k=%d, searched by listed rows" % (
               metric.upper(), args.n, args.vocab, k),
           "dtype": args.dtype, "metric": metric,
           "timing": "host-pointer call to return, wall clock, median of the steps (min next to it)", "clock_mhz": mhz.value,
           "stream_gbs": gbs.value, "steps": args.steps, "warmup": args.warmup, "points": points}
    return res


def grouped(args, metric):
    import time
    import numpy as np
    import torch
    import zvec_amd
    from zvec_amd.index import _np_ptr
    L = zvec_amd._lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    rv = (torch.rand(ri.numel(), generator=g, device=dev) * 2 - 1).cpu()
    np_val = np.float16 if args.dtype == "fp16" else np.float32
    se = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    assert se.reserve(args.n, ri.numel()) == 0
    assert se.add_batch(rc_.numpy().astype(np.uint32), ri.numpy().view(np.uint32), rv.numpy().astype(np_val)) == 0
    del ri, rv
    ctx = se.create_context()
    rng = np.random.default_rng(1)
    ngroups, gnum, gk, k = 1000, 10, 10, 10
    group_of = rng.integers(0, ngroups, args.n).astype(np.uint32)
    fmax = float(np.finfo(np.float32).max)
    before = C.c_int(0)
    assert L.zvec_hip_get_option(b"sparse_group_rows", C.byref(before)) == 0

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), float(min(t))

    points = []
    try:
        for batch in (1, 2, 4, 8, 16, 32, 64):
            qc, qi = zipf_runs(torch, dev, g, batch, 16, 64, args.vocab, 256)
            qv = (torch.rand(qi.numel(), generator=g, device=dev) * 2 - 1).cpu().numpy().astype(np_val)
            qc = qc.numpy().astype(np.uint32)
            qi = qi.numpy().view(np.uint32).copy()
            answers = {}
            point = {"batch": batch}
            for name, width in (("lane_per_query", 0), ("wave_per_row", 64)):
                out = (np.zeros((batch, gnum), np.uint32), np.zeros(batch, np.uint32), np.zeros((batch, gnum, gk), np.uint64),
                       np.zeros((batch, gnum, gk), np.float32), np.zeros((batch, gnum), np.uint32))
                assert L.zvec_hip_set_option(b"sparse_group_rows", width) == 0

                def call():
                    rc = L.zvec_hip_sparse_search_grouped(se._h, ctx._h, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), batch, _np_ptr(group_of),
                                                          ngroups, gnum, gk, fmax, None, *[_np_ptr(a) for a in out])
                    assert rc == 0, rc
                point[name + "_ms"], point[name + "_min_ms"] = median_ms(call)
                answers[name] = out
            keys = np.zeros((batch, k), np.uint64)
            scores = np.zeros((batch, k), np.float32)
            counts = np.zeros(batch, np.uint32)

            def plain():
                rc = L.zvec_hip_sparse_search(se._h, ctx._h, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), batch, k, fmax, None, _np_ptr(keys),
                                              _np_ptr(scores), _np_ptr(counts))
                assert rc == 0, rc
            point["plain_search_ms"], point["plain_search_min_ms"] = median_ms(plain)
            # the two dumps sum the same terms in different orders (agreement_band), place by place
            a, b = answers["lane_per_query"], answers["wave_per_row"]
            assert a[1].tolist() == b[1].tolist() == [gnum] * batch and np.array_equal(a[4], b[4]) and int(a[4].min()) == gk
            point["score_max_abs_diff"] = float(np.abs(a[3] - b[3]).max())
            assert point["score_max_abs_diff"] <= agreement_band(metric)
            point["same_groups"] = float(np.mean(a[0] == b[0]))
            point["same_documents"] = float(np.mean(a[2] == b[2]))
            # the best document overall is the best document of the best group
            assert float(np.abs(a[3][:, 0, 0] - scores[:, 0]).max()) <= agreement_band(metric)
            point["faster"] = "wave_per_row" if point["wave_per_row_ms"] < point["lane_per_query_ms"] else "lane_per_query"
            points.append(point)
            print(json.dumps(point), flush=True)
    finally:
        assert L.zvec_hip_set_option(b"sparse_group_rows", before.value) == 0
    width = 0
    for p in points:                                  # the largest batch up to which the wave-per-row dump won every time
        if p["faster"] != "wave_per_row":
            break
        width = p["batch"]
    res = {"workload": "flat sparse %s %d rows x 64-192 of %d (Zipf), queries 16-64, group-by: %d groups, %d x %d" % (
               metric.upper(), args.n, args.vocab, ngroups, gnum, gk),
           "dtype": args.dtype, "metric": metric, "timing": "host-pointer call to return, wall clock, median of the steps (min next to it)",
           "steps": args.steps, "warmup": args.warmup, "wave_per_row_wins_up_to_batch": width, "points": points}
    return res


def inverted(args, metric):
    import time
    import numpy as np
    import torch
    import zvec_amd
    assert metric == "ip", "the twin serves InnerProductSparse only"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    rv = (torch.rand(ri.numel(), generator=g, device=dev) * 2 - 1).cpu()
    batches = []
    for batch in (1, 64, 1024):
        qc, qi = zipf_runs(torch, dev, g, batch, 16, 64, args.vocab, 256)
        batches.append((batch, qc.numpy().astype(np.uint32), qi.to(dev), torch.rand(qi.numel(), generator=g, device=dev) * 2 - 1))
    ts = torch.cuda.Stream(device=dev)              # (a stream of its own: the null stream would mean "the context's stream")
    ts.wait_stream(torch.cuda.current_stream(dev))
    runs, builds = [], []
    for dtype in ("fp32", "fp16"):
        np_val = np.float16 if dtype == "fp16" else np.float32
        se = zvec_amd.HipFlatSparseStreamer(dtype=dtype)
        assert se.reserve(args.n, ri.numel()) == 0
        assert se.add_batch(rc_.numpy().astype(np.uint32), ri.numpy().view(np.uint32), rv.numpy().astype(np_val)) == 0
        ctx = se.create_context()

        def measure(batch, qc_np, d_qi, qv):
            keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
            scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
            counts = torch.empty((batch,), dtype=torch.int32, device=dev)

            def step():
                rc = se.search_dev(qc_np, d_qi.data_ptr(), qv.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(),
                                   counts.data_ptr(), ctx, stream=ts.cuda_stream)
                assert rc == 0
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(args.steps):
                step()
            e1.record(ts)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps, scores.cpu().numpy(), counts.cpu().numpy()

        legs = []
        for batch, qc_np, d_qi, qv in batches:
            qv = qv.to(torch.float16) if dtype == "fp16" else qv
            ms, scores, counts = measure(batch, qc_np, d_qi, qv)
            legs.append({"batch": batch, "row_scan_ms": ms, "_scores": scores, "_counts": counts, "_q": (qc_np, d_qi, qv)})
        se.set_inverted(True)
        batch, qc_np, d_qi, qv = (legs[0]["batch"],) + legs[0]["_q"]
        keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert se.search_dev(qc_np, d_qi.data_ptr(), qv.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                             ctx, stream=ts.cuda_stream) == 0
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        for leg in legs:
            ms, scores, counts = measure(leg["batch"], *leg.pop("_q"))
            a, ca = leg.pop("_scores"), leg.pop("_counts")
            full = bool(int(counts.min()) == args.topk == int(ca.min())) and bool(np.all(scores[:, 1:] >= scores[:, :-1]))
            leg.update(inverted_ms=ms, score_max_abs_diff=float(np.abs(scores - a).max()),
                       answers_agree=bool(full and float(np.abs(scores - a).max()) <= agreement_band(metric)))
            print(json.dumps(dict(leg, dtype=dtype)), flush=True)
        info = se.inverted_info()
        assert info["builds"] == 1
        runs.append({"dtype": dtype, "elements": se.element_count(), "twin_bytes": info["bytes"], "twin_terms": info["terms"],
                     "tile_rows": info["tile_rows"], "build_ms": first_ms - legs[0]["inverted_ms"], "legs": legs})
        # one build on each route, timed by the library
        L = zvec_amd._lib.lib()
        before = C.c_int(0)
        assert L.zvec_hip_get_option(b"sparse_inverted_build", C.byref(before)) == 0
        build = {"dtype": dtype, "rows": args.n, "elements": se.element_count(), "terms": info["terms"]}
        b_keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        b_scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        b_counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        try:
            for name, route in (("host", 0), ("device", 1)):
                assert L.zvec_hip_set_option(b"sparse_inverted_build", route) == 0
                se.set_inverted(False)
                se.set_inverted(True)
                assert se.search_dev(qc_np, d_qi.data_ptr(), qv.data_ptr(), batch, args.topk, b_keys.data_ptr(), b_scores.data_ptr(),
                                     b_counts.data_ptr(), ctx, stream=ts.cuda_stream) == 0
                torch.cuda.synchronize()
                bi = se.inverted_build_info()
                assert bi["route"] == route and se.inverted_info()["terms"] == info["terms"]
                build[name + "_ms"] = bi["ms"]
                if route:
                    build.update(passes=bi["passes"], block_elems=bi["block_elems"])
        finally:
            assert L.zvec_hip_set_option(b"sparse_inverted_build", before.value) == 0
        width = np.dtype(np_val).itemsize
        per_element = 4 + sum(4 + (4 if p == 0 else 8) + 8 for p in range(build["passes"])) + 4 + 8 + (8 + width) + (4 + width)
        build["device_bytes"] = build["elements"] * per_element + args.n * 8 + build["terms"] * 12
        build["speedup"] = build["host_ms"] / build["device_ms"]
        print(json.dumps(build), flush=True)
        builds.append(build)
        del se, ctx
        torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for b in builds:
        b["bound_ms"] = b["device_bytes"] / (gbs.value * 1e9) * 1e3
        b["bound_fraction"] = b["bound_ms"] / b["device_ms"]
    build_res = {"workload": "term-major twin of flat sparse IP %d rows x 64-192 of %d (Zipf): one build on each route of "
                             "\"sparse_inverted_build\", one process" % (args.n, args.vocab),
                 "timing": "zvec_hip_sparse_inverted_build_info's ms: wall clock of the build inside the first search after the lists were "
                           "dropped and asked for again; one build each, not repeated", "clock_mhz": mhz.value, "stream_gbs": gbs.value,
                 "bound": "device_bytes / stream_gbs (tools/sparse_bench.py, build bytes)", "builds": builds}
    print(json.dumps(build_res))
    if args.build_out:
        with open(args.build_out, "w") as f:
            json.dump(build_res, f, indent=1)
            f.write("\n")
    return {"workload": "flat sparse IP %d rows x 64-192 of %d (Zipf), queries 16-64, k=%d: row scan and inverted lists, one process" % (
                args.n, args.vocab, args.topk),
            "metric": metric, "timing": "device events around the steps of a device-pointer call on a stream; build_ms: wall clock of the "
            "first search after zvec_hip_sparse_set_inverted (the build included) minus a later step", "agreement_band": agreement_band(metric),
            "steps": args.steps, "warmup": args.warmup, "runs": runs}


def put(args, metric):
    import numpy as np
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    rv = (torch.rand(ri.numel(), generator=g, device=dev) * 2 - 1).cpu()
    np_val = np.float16 if args.dtype == "fp16" else np.float32
    width = np.dtype(np_val).itemsize
    counts = rc_.numpy().astype(np.uint32)
    idx, val = ri.numpy().view(np.uint32), rv.numpy().astype(np_val)
    se = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    assert se.add_batch(counts, idx, val) == 0
    twin = None                                   # --from-device: the handle the host entry writes, holding the same corpus
    if args.from_device:
        twin = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
        assert twin.add_batch(counts, idx, val) == 0
    rng = np.random.default_rng(3)
    m = min(args.put_rows, args.n)
    ids = np.sort(rng.choice(args.n, m, replace=False)).astype(np.uint32)

    def rows_of(lengths):
        """rows of the given lengths: indices 0 .. length - 1 (ascending, any length), random values"""
        c = np.asarray(lengths, np.uint32)
        i = np.concatenate([np.arange(x, dtype=np.uint32) for x in c])
        return c, i, rng.uniform(-1, 1, i.size).astype(np_val)
    legs = []
    for name, route, put_ids, lengths in (
            ("in place", 1, ids, counts[ids]),
            ("splice", 2, ids, np.where(counts[ids] > 64, counts[ids] - 1, counts[ids] + 1)),
            ("tail", 0, np.arange(args.n, args.n + m, dtype=np.uint32), np.full(m, 64, np.uint32))):
        c, i, v = rows_of(lengths)
        if twin is None:
            assert se.add_with_id_batch(put_ids, c, i, v) == 0
        else:
            t = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (put_ids, c, i)] + [torch.from_numpy(v).to(dev)]
            torch.cuda.synchronize()
            assert se.put_dev(*t) == 0
        info = se.put_info()
        assert info["route"] == route, (name, info)
        nbytes = info["moved_elems"] * (4 + width)
        legs.append({"route": route, "name": name, "rows": int(m), "ms": info["ms"], "moved_elems": info["moved_elems"],
                     "moved_bytes": nbytes, "moved_gbs": nbytes / info["ms"] / 1e6, "read_and_written_gbs": 2 * nbytes / info["ms"] / 1e6,
                     "elements_after": se.element_count()})
        if twin is not None:
            assert twin.add_with_id_batch(put_ids, c, i, v) == 0
            host = twin.put_info()
            assert host["route"] == route and host["moved_elems"] == info["moved_elems"], (name, host, info)
            legs[-1].update({"entry": "zvec_hip_sparse_put_dev", "host_put_ms": host["ms"], "host_put_moved_gbs": nbytes / host["ms"] / 1e6,
                             "call_pairs": int(i.size)})
        print(json.dumps(legs[-1]), flush=True)
    chunk = se.put_info()["chunk_elems"]
    del se, twin
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    if args.from_device:
        return {"workload": "flat sparse %d rows x 64-192 of %d (Zipf), %s values: one zvec_hip_sparse_put_dev of %d rows on each route, the "
                            "call's rows in device memory; host_put_*: zvec_hip_sparse_put of the same rows on a second handle" % (
                    args.n, args.vocab, args.dtype, m),
                "metric": metric, "timing": "zvec_hip_sparse_put_info's ms: wall clock of the call, its one wait, the plan's upload and the final "
                "drain included (host_put_ms: host checks, staging and both waits included); one call each, not repeated",
                "chunk_elems": chunk, "clock_mhz": mhz.value, "stream_gbs": gbs.value, "legs": legs}
    return {"workload": "flat sparse %d rows x 64-192 of %d (Zipf), %s values: one zvec_hip_sparse_put of %d rows on each route" % (
                args.n, args.vocab, args.dtype, m),
            "metric": metric, "timing": "zvec_hip_sparse_put_info's ms: wall clock of the call, host staging and the waits included; one call "
            "each, not repeated", "chunk_elems": chunk, "clock_mhz": mhz.value, "stream_gbs": gbs.value, "legs": legs}


def ingest(args, metric):
    import time
    import numpy as np
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    tval = torch.float16 if args.dtype == "fp16" else torch.float32
    width = 2 if args.dtype == "fp16" else 4
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(rc_, 0)])

    def dense(counts, idx):
        """the runs scattered into dense rows on the device; values in [0.5, 1): no scattered element is a zero"""
        rows = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts.to(dev))
        m = torch.zeros((counts.numel(), args.vocab), dtype=tval, device=dev)
        m[rows, idx.to(dev).long()] = (torch.rand(idx.numel(), generator=g, device=dev) * 0.5 + 0.5).to(tval)
        return m
    se = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    host = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    blocks, host_blocks = [], []
    for b, a in enumerate(range(0, args.n, args.ingest_rows)):
        z = min(a + args.ingest_rows, args.n)
        m = dense(rc_[a:z], ri[off[a]:off[z]])
        torch.cuda.synchronize()
        assert se.add_dense(m) == 0
        info = se.ingest_info()
        assert info["route"] == 1 and info["elements"] == int(off[z] - off[a]), info
        nbytes = m.numel() * width
        blocks.append({"rows": z - a, "elements": info["elements"], "ms": info["ms"], "matrix_bytes": nbytes,
                       "read_gbs": 2 * nbytes / info["ms"] / 1e6})
        if b < args.ingest_host_blocks:
            t0 = time.perf_counter()
            hm = m.cpu().numpy()
            t1 = time.perf_counter()
            r, c = np.nonzero(hm)
            hc = np.bincount(r, minlength=hm.shape[0]).astype(np.uint32)
            hv = hm[r, c]
            t2 = time.perf_counter()
            assert host.add_batch(hc, c.astype(np.uint32), hv) == 0
            t3 = time.perf_counter()
            host_blocks.append({"rows": z - a, "copy_ms": (t1 - t0) * 1e3, "nonzero_ms": (t2 - t1) * 1e3, "append_ms": (t3 - t2) * 1e3,
                                "ms": (t3 - t0) * 1e3})
        del m
    del host
    searches = []
    for batch in (1, 64, 1024):
        qc, qi = zipf_runs(torch, dev, g, batch, 16, 64, args.vocab, 256)
        qm = dense(qc, qi)
        for _ in range(args.warmup):
            se.search_dense(qm, args.topk)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(torch.cuda.Stream(dev)):
            e0.record()
            for _ in range(args.steps):
                se.search_dense(qm, args.topk)
            e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        searches.append({"batch": batch, "ms": ms, "qps": batch / ms * 1e3, "query_matrix_bytes": qm.numel() * width})
        print(json.dumps(searches[-1]), flush=True)
    slice_cols = se.ingest_info()["slice_cols"]
    rows, elements = se.count(), se.element_count()
    del se
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    dev_ms, mat = sum(b["ms"] for b in blocks), sum(b["matrix_bytes"] for b in blocks)
    res = {"workload": "flat sparse %d rows x 64-192 of %d (Zipf), %s values, as dense device rows in blocks of %d" % (
               args.n, args.vocab, args.dtype, args.ingest_rows),
           "metric": metric, "timing": "appends: zvec_hip_sparse_ingest_info's ms, wall clock of the call, its waits included; searches: "
           "device events around the steps on a stream (each step waits once for the queries' lengths); host route: wall clock",
           "slice_cols": slice_cols, "clock_mhz": mhz.value, "stream_gbs": gbs.value, "rows": rows, "elements": elements,
           "append_dense_ms": dev_ms, "matrix_bytes": mat, "append_dense_read_gbs": 2 * mat / dev_ms / 1e6,
           "append_dense_blocks": len(blocks), "append_dense_block_ms_median": sorted(b["ms"] for b in blocks)[len(blocks) // 2],
           "host_route_blocks": host_blocks, "searches": searches, "steps": args.steps, "warmup": args.warmup}
    if host_blocks:
        res["host_route_ms_per_block"] = sum(b["ms"] for b in host_blocks) / len(host_blocks)
        res["append_dense_ms_per_block_same_blocks"] = sum(b["ms"] for b in blocks[:len(host_blocks)]) / len(host_blocks)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--by-keys", action="store_true")
    ap.add_argument("--grouped", action="store_true")
    ap.add_argument("--inverted", action="store_true")
    ap.add_argument("--put", action="store_true")
    ap.add_argument("--put-rows", type=int, default=1000, help="--put: rows of each call")
    ap.add_argument("--from-device", action="store_true", help="--put: the call's rows in device memory (zvec_hip_sparse_put_dev)")
    ap.add_argument("--ingest", action="store_true")
    ap.add_argument("--ingest-rows", type=int, default=8192, help="--ingest: dense rows generated and appended at a time")
    ap.add_argument("--ingest-host-blocks", type=int, default=4, help="--ingest: blocks that also go the host route")
    ap.add_argument("--build-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "sparse_inverted_build.json"), help="--inverted: where the build timings go")
    ap.add_argument("--dtype", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--metric", choices=("ip", "l2"), default="ip")
    args = ap.parse_args()
    mode, rows = (by_keys, "points") if args.by_keys else (grouped, "points") if args.grouped else (flat, "legs")
    if args.inverted:
        if args.metric != "ip":
            ap.error("--inverted serves InnerProductSparse only")
        mode = inverted
    if args.from_device and not args.put:
        ap.error("--from-device goes with --put")
    if args.put:
        mode = put
        if args.from_device:
            args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparse_put_dev.json")
    if args.ingest:
        mode, rows = ingest, "searches"
        args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparse_ingest.json")
    res = mode(args, "ip")
    if args.metric == "l2":
        res = beside(res, mode(args, "l2"), rows)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def flat(args, metric):
    import numpy as np
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rc_, ri = zipf_runs(torch, dev, g, args.n, 64, 192, args.vocab, 768)
    rv = (torch.rand(ri.numel(), generator=g, device=dev) * 2 - 1).cpu()
    np_val = np.float16 if args.dtype == "fp16" else np.float32
    se = zvec_amd.HipFlatSparseStreamer(dtype=args.dtype, metric=METRIC_NAMES[metric])
    assert se.reserve(args.n, ri.numel()) == 0
    assert se.add_batch(rc_.numpy().astype(np.uint32), ri.numpy().view(np.uint32), rv.numpy().astype(np_val)) == 0
    elements = se.element_count()
    stored = elements * (4 + np.dtype(np_val).itemsize) + (args.n + 1) * 8 + args.n * 8
    ctx = se.create_context()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    legs = []
    for batch in (1, 64, 1024):
        qc, qi = zipf_runs(torch, dev, g, batch, 16, 64, args.vocab, 256)
        qv = torch.rand(qi.numel(), generator=g, device=dev) * 2 - 1
        if args.dtype == "fp16":
            qv = qv.to(torch.float16)              # (the device array search_dev reads: halves for an fp16 index)
        d_qi = qi.to(dev)
        qc_np = qc.numpy().astype(np.uint32)
        keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        ts = torch.cuda.Stream(device=dev)          # (a stream of its own: the null stream would mean "the context's stream")
        ts.wait_stream(torch.cuda.current_stream(dev))
        stream = ts.cuda_stream

        def step():
            rc = se.search_dev(qc_np, d_qi.data_ptr(), qv.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(),
                               counts.data_ptr(), ctx, stream=stream)
            assert rc == 0
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts)
        for _ in range(args.steps):
            step()
        e1.record(ts)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        assert int(counts.min()) == args.topk and bool((scores[:, 1:] >= scores[:, :-1]).all())
        # the host's greedy query blocks (<= 64 queries, <= 4096 elements): probes per stored element, summed over the blocks
        probes, in_blk, elems, longest = 0, 0, 0, 0
        for c in list(qc_np) + [None]:
            if c is None or in_blk == 64 or elems + int(c) > 4096:
                probes += (math.ceil(math.log2(longest)) if longest > 1 else 0) + 1
                in_blk, elems, longest = 0, 0, 0
            if c is not None:
                in_blk, elems, longest = in_blk + 1, elems + int(c), max(longest, int(c))
        legs.append({"batch": batch, "ms_per_step": ms, "qps": batch / ms * 1e3, "probes_per_element": probes})
    del se
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for leg in legs:
        stream_ms = stored / (gbs.value * 1e9) * 1e3
        lds_ms = float(elements) * leg["probes_per_element"] * 2.0 / (cus * mhz.value * 1e6) * 1e3
        leg.update(stream_bound_ms=stream_ms, stream_fraction=stream_ms / leg["ms_per_step"], lds_bound_ms=lds_ms,
                   lds_fraction=lds_ms / leg["ms_per_step"])
    res = {"workload": "flat sparse %s %d rows x 64-192 of %d (Zipf), queries 16-64, k=%d" % (metric.upper(), args.n, args.vocab, args.topk),
           "dtype": args.dtype, "metric": metric,
           "elements": elements, "stored_bytes": stored, "cus": cus, "clock_mhz": mhz.value, "stream_gbs": gbs.value,
           "steps": args.steps, "warmup": args.warmup, "cpu_comparison": "not compared", "legs": legs}
    return res


if __name__ == "__main__":
    main()
