"""HNSW graph search measured (reported, not gated): ms per step, recall@10 against the exact flat search, distances computed per
query, and the gathered bytes per second (distances x row bytes / time) beside the box's calibrated streaming rate.

The corpus is n x dim fp32 from the generator tools/hamming_bench.py --from-fp32 uses.  A real HNSW build at that size is out of
reach of the Python model, so the graph is a k-NN graph made on the GPU with the existing flat search: level 0 holds every row's
m0 / 2 nearest rows plus reverse edges up to m0 = 32; a 1-in-32 sample is level 1, built the same way with m = 16; the entry point
is the sample's first row.

With --build the graph is a real one: zvec_hip_hnsw_build_dev inserts the rows in rounds on the device (m0 32, m 16,
--ef-construction, generated levels), and the result carries the build's seconds, rounds and counters beside the same legs.

    python tools/hnsw_bench.py [--n 1000000 --dim 768] [--out profiles/hnsw_1m.json]
    python tools/hnsw_bench.py --build [--ef-construction 200] [--out profiles/hnsw_build_1m.json]

With --append the first 90 % of the corpus are built and the last 10 % appended (zvec_hip_hnsw_add_dev) in calls of 1, 64 and 4096
rows, each call size on a fresh copy of the 90 % graph: rows per second, device ms of the insert and reverse phases, the share of
rounds that took the one-node path, wall time per call, and recall@10 at ef 128 beside that of one build of all rows.

    python tools/hnsw_bench.py --append [--n 1000000 --dim 768] [--out profiles/hnsw_append_1m.json]

With --dtype fp16 (alone, or with --build or --append) the corpus and the queries are rounded to IEEE binary16 first, and the same
values go through two handles in one process: the fp32 handle (the values widened) and the fp16 handle
(zvec_hip_hnsw_create_typed(ZVEC_HIP_DT_FP16), the halves as they are).  By the contract of DESIGN §3c "fp16 rows" both walk the same
graph to the same answers, so the legs differ in time and in bytes alone: ms per step, QPS and the bytes of rows held are reported
for both, and recall@10 of each against the exact search.  The parent of this option has no fp16 to compare with: the comparison is
fp16 beside fp32 in the same run.

    python tools/hnsw_bench.py --dtype fp16 [--n 100000 --dim 128] [--out profiles/hnsw_1m_fp16.json]
    python tools/hnsw_bench.py --dtype fp16 --build [--out profiles/hnsw_build_1m_fp16.json]
    python tools/hnsw_bench.py --dtype fp16 --append [--out profiles/hnsw_append_1m_fp16.json]
"""
import time
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(torch, stream, steps, warmup, step):
    """ms per step, events on `stream` around `steps` calls"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def knn_dev(torch, zvec_amd, rows, k, stream, chunk=8192):
    """positions of every row's k nearest other rows ([n][k] int64 on the host), by the exact flat search"""
    n, dim = rows.shape
    flat = zvec_amd.HipFlatSearcher(dim, "SquaredEuclidean")
    assert flat.add_batch_dev(rows.data_ptr(), n) == 0
    ctx = flat.create_context()
    dev = rows.device
    keys = torch.empty((chunk, k + 1), dtype=torch.int64, device=dev)
    scores = torch.empty((chunk, k + 1), dtype=torch.float32, device=dev)
    counts = torch.empty((chunk,), dtype=torch.int32, device=dev)
    out = np.zeros((n, k), np.int64)
    torch.cuda.synchronize()
    for o in range(0, n, chunk):
        m = min(chunk, n - o)
        assert flat.search_dev(rows[o:o + m].data_ptr(), m, k + 1, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx, stream=stream) == 0
        torch.cuda.synchronize()
        got = keys[:m].cpu().numpy()
        own = got == np.arange(o, o + m)[:, None]          # a row is its own nearest row: drop it (or the last place on a tie)
        own[~own.any(1), -1] = True
        out[o:o + m] = got[~own].reshape(m, k)
    return out, flat


def with_reverse_edges(knn, cap):
    """lists of up to `cap`: the k forward edges of every node, then reverse edges that are not forward ones, in source order"""
    n, k = knn.shape
    nbr = np.zeros((n, cap), np.uint32)
    nbr[:, :k] = knn
    cnt = np.full(n, k, np.uint32)
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    dst = knn.reshape(-1)
    mutual = np.isin(dst * n + src, src * n + dst)         # dst already lists src
    src, dst = src[~mutual], dst[~mutual]
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    first = np.searchsorted(dst, np.arange(n))
    rank = np.arange(dst.size) - first[dst]
    keep = rank < cap - k
    nbr[dst[keep], k + rank[keep]] = src[keep]
    np.add.at(cnt, dst[keep], 1)
    return nbr, cnt


def append_bench(args, torch, zvec_amd, rows, g, stream, dtype="fp32"):
    """--append (dtype: of the handles; rows and queries hold values of that type, as fp32): 90 % of the corpus built, the last 10 % appended in calls of 1, 64 and 4096 rows, each call size on a fresh copy of
    the 90 % graph (its exported arrays loaded into a new handle); recall@10 at ef 128 beside one build of all rows"""
    n, dim = rows.shape
    m0, m, efc = 32, 16, args.ef_construction
    kw = dict(m=m, m0=m0, ef_construction=efc, scaling_factor=m, seed=1)
    base = n - n // 10
    flat = zvec_amd.HipFlatSearcher(dim, "SquaredEuclidean")
    assert flat.add_batch_dev(rows.data_ptr(), n) == 0
    batch, ef = 1024, 128
    dev = rows.device
    q = torch.randn((batch, dim), generator=g, device=dev, dtype=torch.float32)
    if dtype == "fp16":
        q = q.half().float()
    keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
    scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
    counts = torch.empty((batch,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert flat.search_dev(q.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), flat.create_context(),
                           stream=stream) == 0
    torch.cuda.synchronize()
    truth = keys.cpu().numpy()
    del flat
    if dtype == "fp16":                            # what the handles take: the halves themselves
        rows, q = rows.half(), q.half()

    def recall_of(se):
        assert se.search_dev(q.data_ptr(), batch, args.topk, ef, 0, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), se.create_context(),
                             stream=stream) == 0
        torch.cuda.synchronize()
        got = keys.cpu().numpy()
        return float(np.mean([len(set(got[i]) & set(truth[i])) / float(args.topk) for i in range(batch)]))

    whole = zvec_amd.HipHnswSearcher(dim, "SquaredEuclidean", dtype=dtype)
    t0 = time.perf_counter()
    assert whole.build_dev(rows.data_ptr(), n, **kw) == 0
    one_build = dict(whole.build_info(), build_seconds=time.perf_counter() - t0, recall=recall_of(whole))
    del whole
    part = zvec_amd.HipHnswSearcher(dim, "SquaredEuclidean", dtype=dtype)
    t0 = time.perf_counter()
    assert part.build_dev(rows.data_ptr(), base, **kw) == 0
    part_seconds = time.perf_counter() - t0
    arrays = part.export()
    host_rows = rows[:base].cpu().numpy()
    entry = part.info()["entry_point"]
    del part
    legs = []
    for size in (1, 64, 4096):
        se = zvec_amd.HipHnswSearcher(dim, "SquaredEuclidean", dtype=dtype)
        k_, nbr0, cnt0, upper_of, nbr_up, cnt_up = arrays
        assert se.load(host_rows, nbr0, cnt0, entry, k_, upper_of, nbr_up, cnt_up) == 0
        end = n if size > 1 or args.append_one_rows <= 0 else min(n, base + args.append_one_rows)
        walls, acc = [], dict(rounds=0, rounds_one=0, insert_ms=0.0, reverse_ms=0.0, dists=0, requests=0, prunes=0, grew=0)
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for a in range(base, end, size):
            c = min(size, end - a)
            t0 = time.perf_counter()
            assert se.add_dev(rows[a:a + c].data_ptr(), c, **kw) == 0                  # synchronous
            walls.append(time.perf_counter() - t0)
            i = se.add_info()
            for k in ("rounds", "rounds_one", "insert_ms", "reverse_ms", "dists", "requests", "prunes"):
                acc[k] += i[k]
            acc["grew"] += int(i["grew_rows"] or i["grew_upper"])
        total = time.perf_counter() - t_all
        w = np.array(walls)
        leg = dict(acc, call_rows=size, rows=end - base, calls=len(walls), seconds=total, rows_per_s=(end - base) / total,
                   one_node_share=acc["rounds_one"] / max(acc["rounds"], 1), wall_ms_per_call_mean=float(w.mean() * 1e3),
                   wall_ms_per_call_median=float(np.median(w) * 1e3), wall_ms_per_call_max=float(w.max() * 1e3))
        if end == n:
            leg["recall"] = recall_of(se)
        legs.append(leg)
        del se
    return {"workload": "hnsw append %d x %d %s: %d rows built (m0=%d m=%d ef_construction=%d), %d appended; recall@%d at ef %d, batch %d"
                        % (n, dim, dtype, base, m0, m, efc, n - base, args.topk, ef, batch),
            "measured": "once", "row_bytes_held": n * ((dim + 3) // 4 * 4) * (2 if dtype == "fp16" else 4),
            "build_of_the_first_rows_seconds": part_seconds, "one_build_of_all_rows": one_build, "legs": legs}


def _emit(args, res):
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--append", action="store_true", help="90 %% built, 10 %% appended in calls of 1, 64 and 4096 rows (zvec_hip_hnsw_add_dev)")
    ap.add_argument("--append-one-rows", type=int, default=0, help="rows the one-row-per-call leg appends (0 = the whole 10 %%)")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build", action="store_true", help="build the graph with zvec_hip_hnsw_build_dev instead of the k-NN stand-in")
    ap.add_argument("--ef-construction", type=int, default=200)
    ap.add_argument("--dtype", choices=("fp32", "fp16"), default="fp32",
                    help="fp16: a binary16-representable corpus through the fp32 handle and the fp16 handle, side by side")
    args = ap.parse_args()
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    n, dim, m0, m = args.n, args.dim, 32, 16
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rows = torch.randn((n, dim), generator=g, device=dev, dtype=torch.float32)
    f16 = args.dtype == "fp16"
    if f16:
        rows = rows.half().float()                 # every value is a binary16 value: both handles see the same numbers
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    stream = ts.cuda_stream
    torch.cuda.synchronize()
    if args.append:
        if not f16:
            return _emit(args, append_bench(args, torch, zvec_amd, rows, g, stream))
        state = g.get_state()
        both = {}
        for dt in ("fp32", "fp16"):
            g.set_state(state)                     # (the same queries for both)
            both[dt] = append_bench(args, torch, zvec_amd, rows, g, stream, dt)
        return _emit(args, {"workload": "hnsw append %d x %d, fp16 beside fp32 on one binary16-representable corpus" % (n, dim), **both})
    se = zvec_amd.HipHnswSearcher(dim, "SquaredEuclidean")
    built = None
    if args.build:
        flat = zvec_amd.HipFlatSearcher(dim, "SquaredEuclidean")
        assert flat.add_batch_dev(rows.data_ptr(), n) == 0
        t0 = time.perf_counter()
        assert se.build_dev(rows.data_ptr(), n, m=m, m0=m0, ef_construction=args.ef_construction, seed=1) == 0
        built = dict(se.build_info(), build_seconds=time.perf_counter() - t0, ef_construction=args.ef_construction)
        for name in ("hnsw_build_round_div", "hnsw_build_round_max"):
            v = C.c_int(0)
            assert zvec_amd._lib.lib().zvec_hip_get_option(name.encode(), C.byref(v)) == 0
            built[name] = v.value
    else:
        knn0, flat = knn_dev(torch, zvec_amd, rows, m0 // 2, stream)
        nbr0, cnt0 = with_reverse_edges(knn0, m0)
        sample = np.arange(0, n, 32)
        knn1, _ = knn_dev(torch, zvec_amd, rows[::32].contiguous(), min(m // 2, sample.size - 1), stream)
        nbr1, cnt1 = with_reverse_edges(knn1, m)
        upper_of = np.full(n, 0xffffffff, np.uint32)
        upper_of[sample] = np.arange(sample.size, dtype=np.uint32)
        nbr_up = sample[nbr1.astype(np.int64)].astype(np.uint32).reshape(sample.size, 1, m)
        assert se.load(rows.cpu().numpy(), nbr0, cnt0, 0, None, upper_of, nbr_up, cnt1.reshape(-1, 1)) == 0
    handles = [("fp32", se, 4)]
    if f16:
        # the same graph in an fp16 handle: what the fp32 handle exports, over the halves (with --build the contract says a build of
        # the halves gives this graph; loading it keeps the bench to one build)
        se16 = zvec_amd.HipHnswSearcher(dim, "SquaredEuclidean", dtype="fp16")
        k_, nbr0_, cnt0_, upper_of_, nbr_up_, cnt_up_ = se.export()
        assert se16.load(rows.half().cpu().numpy(), nbr0_, cnt0_, se.info()["entry_point"], k_, upper_of_, nbr_up_, cnt_up_) == 0
        handles.append(("fp16", se16, 2))
        del k_, nbr0_, cnt0_, upper_of_, nbr_up_, cnt_up_
    fctx = flat.create_context()
    legs = []
    for batch in (1, 64, 1024):
        q = torch.randn((batch, dim), generator=g, device=dev, dtype=torch.float32)
        if f16:
            q = q.half().float()
        keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        exact = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert flat.search_dev(q.data_ptr(), batch, args.topk, exact.data_ptr(), scores.data_ptr(), counts.data_ptr(), fctx, stream=stream) == 0
        torch.cuda.synchronize()
        truth = exact.cpu().numpy()
        for ef in (64, 128, 256):
            for name, hs, esz in handles:
                hq = q.half() if esz == 2 else q
                hctx = hs.create_context()

                def step():
                    assert hs.search_dev(hq.data_ptr(), batch, args.topk, ef, 0, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), hctx,
                                         stream=stream) == 0
                ms = _timed(torch, ts, args.steps, args.warmup, step)
                scanned, hops, _ = hs.last_stats(hctx, batch)
                got = keys.cpu().numpy()
                recall = float(np.mean([len(set(got[i]) & set(truth[i])) / float(args.topk) for i in range(batch)]))
                gathered = float(scanned.sum()) * dim * esz
                leg = {"batch": batch, "ef": ef, "ms_per_step": ms, "qps": batch / ms * 1e3, "recall_at_%d" % args.topk: recall,
                       "mean_scanned": float(scanned.mean()), "mean_hops": float(hops.mean()), "gathered_gbs": gathered / ms / 1e6}
                if f16:
                    leg = dict(dtype=name, row_bytes_held=n * ((dim + 3) // 4 * 4) * esz, **leg)
                legs.append(leg)
    del rows, flat
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for leg in legs:
        leg["stream_fraction"] = leg["gathered_gbs"] / gbs.value
    graph = "graph built on the device m0=%d m=%d" % (m0, m) if args.build else "k-NN graph m0=%d (+ 1-in-32 level 1, m=%d)" % (m0, m)
    what = "fp16 beside fp32 on one binary16-representable corpus" if f16 else "fp32"
    res = {"workload": "hnsw search %d x %d %s, %s, k=%d" % (n, dim, what, graph, args.topk),
           "stream_gbs": gbs.value, "clock_mhz": mhz.value, "steps": args.steps, "warmup": args.warmup, "legs": legs}
    if built is not None:
        res["build"] = built
    _emit(args, res)


if __name__ == "__main__":
    main()
