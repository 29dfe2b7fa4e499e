"""Flat Hamming search, 1M x 768 bits, k = 10, batches 1 / 256 / 1024: QPS and ms per step against two bounds of the box it
runs on (reported, not gated; bench.py is the project's benchmark and does not cover binary rows).

  streaming bound  stored bytes of the index / the box's streaming figure (zvec_hip_calibrate, same process): batch 1
  VALU bound       2 vector-ALU instructions (v_xor_b32 + v_bcnt_u32_b32) per 32-bit word pair; a wave64 instruction issues in
                   2 cycles on a SIMD, i.e. 32 word pairs per cycle and SIMD; 4 SIMDs x CUs; at the calibrated shader clock

    python tools/hamming_bench.py [--out profiles/hamming_flat1m_768b.json] [--steps 20] [--warmup 5]
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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
