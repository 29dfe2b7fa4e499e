"""Flat Hamming search, 1M x 768 bits, k = 10, batches 1 / 256 / 1024: QPS and ms per step against two bounds of the box it
runs on (reported, not gated; bench.py is the project's benchmark and does not cover binary rows).

  streaming bound  stored bytes of the index / the box's streaming figure (zvec_hip_calibrate, same process): batch 1
  VALU bound       2 vector-ALU instructions (v_xor_b32 + v_bcnt_u32_b32) per 32-bit word pair; a wave64 instruction issues in
                   2 cycles on a SIMD, i.e. 32 word pairs per cycle and SIMD; 4 SIMDs x CUs; at the calibrated shader clock

    python tools/hamming_bench.py [--out profiles/hamming_flat1m_768b.json] [--steps 20] [--warmup 5]

--from-fp32 measures the index fed with fp32 embeddings instead (n x bits fp32 values turned into sign bits on the GPU): the encoder
alone and the fp32 append in GB/s of fp32 input against the box's streaming figure of the same run, and search_fp32 beside the
bit-fed search at the same batches.  Reported, not gated.

    python tools/hamming_bench.py --from-fp32 [--out profiles/hamming_from_fp32.json]

--ivf measures the same rows through inverted lists (zvec_hip_bivf_*): the index is built with nlist 1024 on the GPU, batches 1 / 256 /
1024 are timed at nprobe 8 / 32 / 128 next to the flat scan of the same rows IN THE SAME PROCESS — the yardstick —, with recall@10
against the flat answer (tie-aware: a returned score at or below the flat k-th score counts), the bytes of the probed lists per step
over the box's streaming figure, and the build time.  The rows are 1024 random prototypes with one bit in eight flipped at random, so
that there is something to cluster.  Reported, not gated.

    python tools/hamming_bench.py --ivf [--out profiles/hamming_ivf.json]

--ivf --from-fp32 generates the --ivf corpus as fp32 (1024 normal prototypes plus noise that flips one sign in eight), builds it with
zvec_hip_bivf_build_fp32_dev and times search_fp32 at batches 1 / 256 / 1024, k = 10, refine 1 / 2 / 4 / 8 / 12: QPS, recall@10
against an exact fp32 flat search of the same rows, and the re-rank's time (the fp32 search minus the bit-fed search at topk = kc,
which also holds the query encoder) beside the bound its gathered bytes set at the box's streaming figure.  Reported, not gated.

    python tools/hamming_bench.py --ivf --from-fp32 [--out profiles/hamming_ivf_fp32.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=768)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--from-fp32", action="store_true", help="feed the index with fp32 rows / queries (encoder, fp32 append, search_fp32)")
    ap.add_argument("--ivf", action="store_true", help="the rows through inverted lists next to the flat scan (zvec_hip_bivf_*)")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--kmeans-iters", type=int, default=5)
    ap.add_argument("--nprobe", type=int, default=32, help="--ivf --from-fp32: lists probed")
    args = ap.parse_args()
    if args.ivf and args.from_fp32:
        return ivf_fp32(args)
    if args.from_fp32:
        return from_fp32(args)
    if args.ivf:
        return ivf(args)
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    words = args.bits // 32
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    base = torch.randint(-2**31, 2**31 - 1, (args.n, words), generator=g, device=dev, dtype=torch.int32)
    se = zvec_amd.HipFlatSearcher(args.bits, "Hamming", dtype="binary32")
    torch.cuda.synchronize()
    assert se.add_batch_dev(base.data_ptr(), args.n) == 0
    ctx = se.create_context()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    chunks = (words + 3) // 4
    stored = (args.n + 127) // 128 * 128 * chunks * 16
    legs = []
    for batch in (1, 256, 1024):
        q = torch.randint(-2**31, 2**31 - 1, (batch, words), generator=g, device=dev, dtype=torch.int32)
        keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        ts = torch.cuda.Stream(device=dev)          # (a stream of its own: the null stream would mean "the context's stream")
        ts.wait_stream(torch.cuda.current_stream(dev))
        stream = ts.cuda_stream

        def step():
            rc = se.search_dev(q.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx, stream=stream)
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
        legs.append({"batch": batch, "ms_per_step": ms, "qps": batch / ms * 1e3})
    del base
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for leg in legs:
        stream_ms = stored / (gbs.value * 1e9) * 1e3
        pairs = float(leg["batch"]) * args.n * words
        valu_ms = pairs / (32.0 * 4 * cus * mhz.value * 1e6) * 1e3
        leg.update(stream_bound_ms=stream_ms, stream_fraction=stream_ms / leg["ms_per_step"], valu_bound_ms=valu_ms,
                   valu_fraction=valu_ms / leg["ms_per_step"])
    res = {"workload": "flat hamming %d x %d bits, k=%d" % (args.n, args.bits, args.topk), "stored_bytes": stored, "cus": cus,
           "clock_mhz": mhz.value, "stream_gbs": gbs.value, "steps": args.steps, "warmup": args.warmup, "legs": legs}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


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


def from_fp32(args):
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    n, dim, words = args.n, args.bits, (args.bits + 31) // 32
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rows = torch.randn((n, dim), generator=g, device=dev, dtype=torch.float32)
    in_bytes = float(n) * dim * 4
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    stream = ts.cuda_stream
    ectx = zvec_amd.IndexContext(0)
    enc_out = torch.empty((n, words), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    enc_ms = _timed(torch, ts, args.steps, args.warmup,
                    lambda: ectx.binary_encode_dev(rows.data_ptr(), n, dim, enc_out.data_ptr(), stream=stream))

    # the fp32 append (encode + pack into the blocked layout), a fresh index per step; reserved, so no growth copy is timed
    def fresh():
        se = zvec_amd.HipFlatSearcher(words * 32, "Hamming", dtype="binary32")
        assert se.reserve(n) == 0
        return se
    app = []
    for _ in range(max(2, min(args.steps, 5))):
        se = fresh()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts)
        assert se.add_batch_fp32_dev(rows.data_ptr(), n, dim, stream=stream) == 0
        e1.record(ts)
        torch.cuda.synchronize()
        app.append(e0.elapsed_time(e1))
    app_ms = min(app[1:])
    ctx = se.create_context()
    legs = []
    for batch in (1, 256, 1024):
        q = torch.randn((batch, dim), generator=g, device=dev, dtype=torch.float32)
        qw = torch.empty((batch, words), dtype=torch.int32, device=dev)
        keys = torch.empty((batch, args.topk), dtype=torch.int64, device=dev)
        scores = torch.empty((batch, args.topk), dtype=torch.float32, device=dev)
        counts = torch.empty((batch,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ectx.binary_encode_dev(q.data_ptr(), batch, dim, qw.data_ptr(), stream=stream)

        def fp32_step():
            assert se.search_fp32_dev(q.data_ptr(), dim, batch, args.topk, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx,
                                      stream=stream) == 0

        def bits_step():
            assert se.search_dev(qw.data_ptr(), batch, args.topk, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx, stream=stream) == 0
        ms_fp32 = _timed(torch, ts, args.steps, args.warmup, fp32_step)
        fp32_scores = scores.clone()
        ms_bits = _timed(torch, ts, args.steps, args.warmup, bits_step)
        assert int(counts.min()) == args.topk and bool((scores == fp32_scores).all())
        legs.append({"batch": batch, "search_fp32_ms": ms_fp32, "search_fp32_qps": batch / ms_fp32 * 1e3, "search_bits_ms": ms_bits,
                     "search_bits_qps": batch / ms_bits * 1e3})
    del rows, enc_out, se
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    enc_gbs, app_gbs = in_bytes / enc_ms / 1e6, in_bytes / app_ms / 1e6
    res = {"workload": "flat hamming fed with fp32: %d x %d values, k=%d" % (n, dim, args.topk), "input_bytes": in_bytes,
           "stream_gbs": gbs.value, "clock_mhz": mhz.value, "steps": args.steps, "warmup": args.warmup,
           "encode": {"ms": enc_ms, "input_gbs": enc_gbs, "stream_fraction": enc_gbs / gbs.value},
           "append_fp32": {"ms": app_ms, "input_gbs": app_gbs, "stream_fraction": app_gbs / gbs.value},
           "legs": legs}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def ivf(args):
    import time
    import numpy as np
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    n, words, k = args.n, args.bits // 32, args.topk
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def rand(rows):
        return torch.randint(-2**31, 2**31 - 1, (rows, words), generator=g, device=dev, dtype=torch.int32)

    def noisy(src):                                   # one bit in eight flipped
        return src ^ (rand(src.shape[0]) & rand(src.shape[0]) & rand(src.shape[0]))
    proto = rand(1024)
    base = noisy(proto[torch.randint(0, 1024, (n,), generator=g, device=dev)])
    flat = zvec_amd.HipFlatSearcher(args.bits, "Hamming", dtype="binary32")
    se = zvec_amd.HipHammingIVFSearcher(args.bits, dtype="binary32")
    torch.cuda.synchronize()
    assert flat.add_batch_dev(base.data_ptr(), n) == 0
    t0 = time.perf_counter()
    assert se.build_dev(base.data_ptr(), n, args.nlist, kmeans_iters=args.kmeans_iters) == 0
    build_s = time.perf_counter() - t0
    ctx = se.create_context()
    row_bytes = (words + 3) // 4 * 16
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    stream = ts.cuda_stream
    legs = []
    for batch in (1, 256, 1024):
        q = noisy(base[torch.randint(0, n, (batch,), generator=g, device=dev)])
        out = [(torch.empty((batch, k), dtype=torch.int64, device=dev), torch.empty((batch, k), dtype=torch.float32, device=dev),
                torch.empty((batch,), dtype=torch.int32, device=dev)) for _ in range(2)]
        (fk, fs, fc), (ik, is_, ic) = out
        torch.cuda.synchronize()
        flat_ms = _timed(torch, ts, args.steps, args.warmup, lambda: flat.search_dev(
            q.data_ptr(), batch, k, fk.data_ptr(), fs.data_ptr(), fc.data_ptr(), ctx, stream=stream))
        for nprobe in (8, 32, 128):
            ms = _timed(torch, ts, args.steps, args.warmup, lambda: se.search_dev(
                q.data_ptr(), batch, k, nprobe, 0xffffffff, ik.data_ptr(), is_.data_ptr(), ic.data_ptr(), ctx, stream=stream))
            _, _, scanned = se.last_probes(ctx, batch, nprobe)
            hit = (is_ <= fs[:, k - 1:k]) & (torch.arange(k, device=dev)[None, :] < ic[:, None])
            legs.append({"batch": batch, "nprobe": nprobe, "ms_per_step": ms, "qps": batch / ms * 1e3, "flat_ms_per_step": flat_ms,
                         "flat_qps": batch / flat_ms * 1e3, "recall_at_k": float(hit.sum()) / (batch * k),
                         "probed_bytes": float(scanned.astype(np.float64).sum()) * row_bytes})
    del base
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for leg in legs:
        leg["stream_bound_ms"] = leg["probed_bytes"] / (gbs.value * 1e9) * 1e3
        leg["stream_fraction"] = leg["stream_bound_ms"] / leg["ms_per_step"]
    res = {"workload": "hamming ivf %d x %d bits, nlist=%d, k=%d" % (n, args.bits, args.nlist, k), "build_seconds": build_s,
           "kmeans_iters": args.kmeans_iters, "stream_gbs": gbs.value, "clock_mhz": mhz.value, "steps": args.steps, "warmup": args.warmup,
           "legs": legs}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def ivf_fp32(args):
    import time
    import torch
    import zvec_amd
    dev = torch.device("cuda:0")
    n, dim, k = args.n, args.bits, args.topk
    words = (dim + 31) // 32
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sigma = 0.41421356                                # tan(pi / 8): one sign in eight flips, as one bit in eight of --ivf

    def noisy(src):
        return src + sigma * torch.randn(src.shape, generator=g, device=dev, dtype=torch.float32)
    proto = torch.randn((1024, dim), generator=g, device=dev, dtype=torch.float32)
    base = noisy(proto[torch.randint(0, 1024, (n,), generator=g, device=dev)])
    exact = zvec_amd.HipFlatSearcher(dim, "SquaredEuclidean")
    se = zvec_amd.HipHammingIVFSearcher(words * 32, dtype="binary32")
    torch.cuda.synchronize()
    assert exact.add_batch_dev(base.data_ptr(), n) == 0
    t0 = time.perf_counter()
    assert se.build_fp32_dev(base.data_ptr(), n, dim, args.nlist, "SquaredEuclidean", kmeans_iters=args.kmeans_iters) == 0
    build_s = time.perf_counter() - t0
    del base                                          # (both indexes hold their copy)
    ctx, ectx = se.create_context(), exact.create_context()
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    stream = ts.cuda_stream
    nprobe = args.nprobe
    legs = []
    for batch in (1, 256, 1024):
        q = noisy(proto[torch.randint(0, 1024, (batch,), generator=g, device=dev)])
        qw = torch.empty((batch, words), dtype=torch.int32, device=dev)
        ek, es, ec = (torch.empty((batch, k), dtype=torch.int64, device=dev), torch.empty((batch, k), dtype=torch.float32, device=dev),
                      torch.empty((batch,), dtype=torch.int32, device=dev))
        rk, rs, rc_ = torch.full_like(ek, -1), torch.empty_like(es), torch.empty_like(ec)
        torch.cuda.synchronize()
        assert exact.search_dev(q.data_ptr(), batch, k, ek.data_ptr(), es.data_ptr(), ec.data_ptr(), ectx, stream=stream) == 0
        ctx.binary_encode_dev(q.data_ptr(), batch, dim, qw.data_ptr(), stream=stream)
        for refine in (1, 2, 4, 8, 12):
            kc = min(k * refine, 128)
            hk, hs = torch.empty((batch, kc), dtype=torch.int64, device=dev), torch.empty((batch, kc), dtype=torch.float32, device=dev)
            rk.fill_(-1)
            ms = _timed(torch, ts, args.steps, args.warmup, lambda: se.search_fp32_dev(
                q.data_ptr(), dim, batch, k, refine, nprobe, 0xffffffff, rk.data_ptr(), rs.data_ptr(), rc_.data_ptr(), ctx, stream=stream))
            hit = (rk[:, :, None] == ek[:, None, :]).any(dim=2) & (torch.arange(k, device=dev)[None, :] < rc_[:, None])
            # stage 1 alone at the same width: the bit-fed search with topk = kc; the difference is the encoder plus the re-rank
            ms_bits = _timed(torch, ts, args.steps, args.warmup, lambda: se.search_dev(
                qw.data_ptr(), batch, kc, nprobe, 0xffffffff, hk.data_ptr(), hs.data_ptr(), rc_.data_ptr(), ctx, stream=stream))
            legs.append({"batch": batch, "refine": refine, "kc": kc, "nprobe": nprobe, "ms_per_step": ms, "qps": batch / ms * 1e3,
                         "recall_at_k": float(hit.sum()) / (batch * k), "stage1_ms_per_step": ms_bits,
                         "rerank_ms_estimate": ms - ms_bits, "gathered_bytes": float(batch) * kc * dim * 4})
    del exact
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info(dev)
    nbytes = int(min(30e9, free * 0.8)) // 4096 * 4096
    mhz, gbs = C.c_double(0), C.c_double(0)
    rc = zvec_amd._lib.lib().zvec_hip_calibrate(0, None, nbytes, 3, C.byref(mhz), C.byref(gbs))
    assert rc == 0, rc
    for leg in legs:
        leg["rerank_stream_bound_ms"] = leg["gathered_bytes"] / (gbs.value * 1e9) * 1e3
    res = {"workload": "hamming ivf fed with fp32: %d x %d values, nlist=%d, nprobe=%d, k=%d, re-ranked by squared L2" % (n, dim, args.nlist, nprobe, k),
           "build_seconds": build_s, "kmeans_iters": args.kmeans_iters, "rows_bytes": float(n) * dim * 4, "stream_gbs": gbs.value,
           "clock_mhz": mhz.value, "steps": args.steps, "warmup": args.warmup, "legs": legs}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
