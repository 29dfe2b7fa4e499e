"""GPU test: handles give back the device memory they took — run with -m gpu.

Two loops of 16 create / use / destroy cycles each, free device memory read before and after each loop: a control loop that only
creates and destroys an empty sharded handle, and a work loop that takes every index kind through the paths that replace or drop
device arrays.  Before device allocations had one owner each, zvec_hip_shards_destroy forgot the per-shard probe lists of a dealt
coarse pass: 2 shards x 16 cycles x ((4096 x 64 + 4096) x 4 x 1.25 + 256) bytes = 42.6 MB stayed behind in the work loop.

The assertion is drop(work) <= drop(control) + margin, the margin a quarter of that leak (10.65 MB).  Measured on an MI355X, where
free memory moves in steps of 2 MiB (so every 1.33 MB probe list cost 2 MiB):
    before the change   drop(control) = 0 B, drop(work) = 67 108 864 B   (32 lists x 2 MiB; the test fails)
    with it             drop(control) = 0 B, drop(work) = 0 B

The warm-up runs the work cycle twice.  The HIP runtime takes memory of its own once, at the second sharded search of a process, and
keeps it: 32 MiB with 4 hardware queues (16 MiB with 2, nothing with 8 or 16), then not a byte over 32 further cycles.  After a
single warm-up cycle that step falls into the work loop and reads as 33 554 432 B lost by handles that had lost nothing.
"""
import gc

import numpy as np
import pytest

from tests.util import kmeans_lists, ivf_search, flat_search

pytestmark = pytest.mark.gpu

CYCLES = 16
DEALT_Q, DEALT_NPROBE, SHARDS = 4096, 64, 2
PROBE_LIST_BYTES = (DEALT_Q * DEALT_NPROBE + DEALT_Q) * 4 * 5 // 4 + 256      # one shard's, as DevBuf sizes it
MARGIN = SHARDS * CYCLES * PROBE_LIST_BYTES // 4


def _free_bytes():
    import torch
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _control_cycle(zv, dim):
    sh = zv.HipShardedIndex("ivf", dim, "SquaredEuclidean", devices=[0] * SHARDS)
    del sh


def _work_cycle(zv, data):
    base, cent, offs, order, q_wide, q = data
    dim = base.shape[1]
    # a sharded IVF index whose coarse pass is dealt over the shards
    sh = zv.HipShardedIndex("ivf", dim, "SquaredEuclidean", devices=[0] * SHARDS)
    assert sh.load(cent, offs, base[order], order.astype(np.uint64)) == 0
    assert sh.deal_coarse(True) == 0
    sh.search(q_wide, 10, nprobe=DEALT_NPROBE, max_scan=len(base))
    del sh
    # a flat index with a twin: searched, appended to (drops the twin), searched again
    fl = zv.HipFlatStreamer(dim, "SquaredEuclidean")
    assert fl.add_batch(base[:20000]) == 0
    fl.set_shadow(True)
    flat_search(fl, q, 10)
    assert fl.add_batch(base[20000:]) == 0
    assert not fl.shadow_info()["enabled"]
    flat_search(fl, q, 10)
    del fl
    # an IVF index built, given a twin, searched, and built again (lists, tables and twin are replaced)
    se = zv.HipIVFSearcher(dim, "SquaredEuclidean")
    assert se.build(base, 128, kmeans_iters=2, sample_per_list=64, seed=7) == 0
    se.set_shadow(True)
    ivf_search(se, q, 10)
    assert se.build(base, 128, kmeans_iters=2, sample_per_list=64, seed=8) == 0
    del se


def test_handles_give_back_their_device_memory():
    import zvec_amd as zv
    rng = np.random.default_rng(77)
    n, dim, nlist = 30000, 40, 128
    base = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    cent, offs, order = kmeans_lists(rng, base, nlist)
    data = (base, np.round(cent), offs, order, rng.integers(-8, 9, (DEALT_Q, dim)).astype(np.float32),
            rng.integers(-8, 9, (64, dim)).astype(np.float32))
    _control_cycle(zv, dim)                     # warm-up: runtime, code objects, and the runtime's one-time step (see above)
    _work_cycle(zv, data)
    _work_cycle(zv, data)
    before = _free_bytes()
    for _ in range(CYCLES):
        _control_cycle(zv, dim)
    drop_control = before - _free_bytes()
    before = _free_bytes()
    for _ in range(CYCLES):
        _work_cycle(zv, data)
    drop_work = before - _free_bytes()
    print("free device memory lost over %d cycles: control %d B, work %d B (margin %d B)" % (CYCLES, drop_control, drop_work, MARGIN))
    assert drop_work <= drop_control + MARGIN
