"""IVF build labelling (assign_kernel<F16>, assign256_f16_kernel<L2>) and the k-means step (centroid_mean_kernel<F16>, ivf_train)
on REAL-VALUED data against plain fp64 — run with -m gpu.

test_gpu_build.py pins these kernels where every score is exact (small integers).  That catches indexing mistakes; it cannot catch
a stale |x|^2 or |c|^2, a norm read for the wrong column, an accumulator that survives a tile fold, a narrower accumulation, a pad
column that wins when real scores are large, or a mean that drifts.  Here every label is held to the fp64 arg-min through the
derived band of tests/util.py label_reference (acceptance rule + no more differences than ambiguous rows + at most 1 % of the rows
ambiguous), every mean to the fp64 mean through the bound of a sequential fp32 sum.  Every fourth row of every case sits 3-30
bands from the bisector of its two nearest centroids (tests/util.py label_steer): those rows are what the band decides, and
tests/test_label_reference_cpu.py shows that an accumulation error of half precision fails on them up to a scan width of 256.

Dispatch (ivf_label_rows): fp32 rows always take assign_kernel<false>; fp16 rows take the 256 x 256 tile iff option assign256 != 0
and rows >= 512 and centroids >= 192 and nks >= 2, else assign_kernel<true>.  nks = k-steps per row: ceil(d / 32) for fp32,
ceil(d / 64) for fp16.  Step counts: 128 tile nsteps = ceil(n / 128) * nks; 256 tile nsteps = ceil(ceil(n / 128) / 2) * nks.
What each shape of tests.util.LABEL_SHAPES hits (rows, centroids, dim):

  shape              fp32 assign_kernel<false>      fp16, assign256 = 1                          fp16, assign256 = 0
  (1, 1, 1)          1 step (single)                128 tile, 1 step                             same
  (127, 2, 31)       1 step, ragged item            128 tile, 1 step                             same
  (128, 63, 32)      1 step, one full item          128 tile, 1 step                             same
  (129, 64, 33)      2 steps, 2 items (1 row)       128 tile, 1 step                             same
  (511, 127, 64)     2 steps                        128 tile, 1 step (rows < 512)                same
  (512, 128, 65)     3 steps (ODD: loop breaks)     128 tile, 2 steps (centroids < 192)          same
  (513, 129, 100)    8 steps, 2nd tile 1 column     128 tile, 4 steps                            same
  (767, 191, 128)    8 steps                        128 tile, 4 steps (191 < 192)                same
  (512, 192, 65)     6 steps                        256 tile, nsteps 2 (MINIMUM), 2nd tile half  128 tile, 4 steps
  (513, 193, 128)    8 steps                        256 tile, nsteps 2, last item moved back     128 tile, 4 steps
  (1025, 255, 129)   10 steps                       256 tile, 3 steps (odd), pad column 255      128 tile, 6 steps
  (767, 256, 100)    8 steps                        256 tile, nsteps 2, one full pair            128 tile, 4 steps
  (511, 256, 128)    8 steps                        128 tile, 4 steps (rows < 512)               same
  (1025, 383, 31)    3 steps (ODD)                  128 tile, 3 steps (ODD; nks 1 < 2)           same
  (640, 383, 65)     9 steps (ODD)                  256 tile, 4 steps, 2nd tile of pair 2 MISSING 128 tile, 6 steps
  (600, 385, 129)    20 steps                       256 tile, 6 steps, last tile 1 column        128 tile, 12 steps
  (2500, 385, 64)    8 steps                        128 tile, 4 steps (nks 1)                    same
  (4000, 1000, 33)   16 steps                       128 tile, 8 steps                            same
  (2049, 1000, 100)  32 steps                       256 tile, 8 steps, 4 pairs                   128 tile, 16 steps
  (3000, 257, 768)   72 steps                       256 tile, 24 steps, 2nd tile missing         128 tile, 36 steps
(step counts for SquaredEuclidean / InnerProduct; cosine rows scan one float or two halves fewer).  Batch edge (2^18 rows per
batch): see test_batch_edge."""
import ctypes as C

import numpy as np
import pytest

from tests import util as U

pytestmark = pytest.mark.gpu

IDX_NONE = 0xffffffff
BATCH = 1 << 18


@pytest.fixture(scope="module")
def zv():
    import zvec_amd
    return zvec_amd


def _npdt(dtype):
    return np.float16 if dtype == "fp16" else np.float32


def _label(se, d_rows, n):
    import torch
    d_lab = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    assert se.label_dev(d_rows.data_ptr(), n, d_lab.data_ptr()) == 0
    torch.cuda.synchronize()
    return d_lab.cpu().numpy().view(np.uint32).astype(np.int64)


def _gpu_labels(zv, cent, rows, metric, dtype):
    """labels of `rows` under `cent` through set_centroids + label_dev: one array for fp32; for fp16 one per setting of the
    assign256 option, (1, 0) in that order, the option restored to 1"""
    import torch
    from zvec_amd import _lib
    L = _lib.lib()
    se = zv.HipIVFSearcher(cent.shape[1], metric, dtype=dtype)
    assert se.set_centroids(cent) == 0
    d_rows = torch.from_numpy(rows).cuda()
    if dtype != "fp16":
        return [_label(se, d_rows, len(rows))]
    out = []
    try:
        for opt in (1, 0):
            assert L.zvec_hip_set_option(b"assign256", opt) == 0
            out.append(_label(se, d_rows, len(rows)))
    finally:
        assert L.zvec_hip_set_option(b"assign256", 1) == 0
    return out


def _check_both(cent, rows, metric, labs, ignore, what, cap=0.01, ref=None):
    """each tile's labels independently; where the gap exceeds the band the two tiles must agree with each other"""
    for t, lab in enumerate(labs):
        ref = U.check_labels(cent, rows, metric, lab, ignore, cap=cap, what="%s [labels %d]" % (what, t), ref=ref)
    if len(labs) == 2:
        clear = ~U.label_ambiguous(*ref, ignore)
        assert np.array_equal(labs[0][clear], labs[1][clear]), what
    return ref


@pytest.mark.parametrize("shape", U.LABEL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dtype,kind", U.LABEL_KINDS)
def test_real_valued_labels_against_fp64(zv, dtype, kind, shape):
    """every metric label_dev accepts.  Cosine on the plain means only, where the row is wide enough to carry its norm slots:
    cosine rows and centroids are unit vectors, so the per-tile scaling of "tiles" and the magnitudes of "big" do not exist."""
    rows, nlist, dim = shape
    metrics = ["SquaredEuclidean", "InnerProduct"] + (["Cosine"] if kind == "means" and dim >= 31 else [])
    for metric in metrics:
        cent, x, ignore = U.label_case(rows, nlist, dim, _npdt(dtype), kind, metric)
        labs = _gpu_labels(zv, cent, x, metric, dtype)
        _check_both(cent, x, metric, labs, ignore, "%s %s %s %r" % (dtype, kind, metric, shape))


def test_labelling_is_refused_while_a_separate_coarse_space_is_installed(zv):
    import torch
    from zvec_amd import _lib
    L = _lib.lib()
    se = zv.HipIVFSearcher(32, "InnerProduct")
    cent = np.random.default_rng(2).standard_normal((8, 36)).astype(np.float32)
    assert L.zvec_hip_ivf_set_coarse_space(se._h, 36, 0, cent.ctypes.data_as(C.c_void_p), 8) == 0
    d = torch.zeros((16, 32), device="cuda")
    lab = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert se.label_dev(d.data_ptr(), 16, lab.data_ptr()) == zv.IndexError_.Unsupported
    assert se.set_centroids(cent[:, :32]) == 0                       # back in the rows' own space
    assert se.label_dev(d.data_ptr(), 16, lab.data_ptr()) == 0


# (index type, rows, centroids, dim): what the two batches of the one label_dev call take
#   fp32 2^18 + 300, 300, 64   assign_kernel<false>, 6 steps; second batch 300 rows = 3 items, the last of 44 rows
#   fp32 2^18 + 513, 300, 64   the same kernel; second batch 513 rows = 5 items, the last of ONE row
#   fp16 2^18 + 513, 300, 64   nks 1: the 128 tile in both batches (both option settings the same path), second batch 513 rows
#   fp16 2^18 + 300, 200, 72   nks 2: the 256 tile for the full batch, the 128 tile for the 300 rows left (< 512) — in ONE call
#   fp16 2^18 + 513, 200, 72   the 256 tile for both; the second batch's last item (1 row of its own) is moved back
@pytest.mark.parametrize("dtype,rows,nlist,dim", [("fp32", BATCH + 300, 300, 64), ("fp32", BATCH + 513, 300, 64),
                                                  ("fp16", BATCH + 513, 300, 64), ("fp16", BATCH + 300, 200, 72),
                                                  ("fp16", BATCH + 513, 200, 72)])
def test_batch_edge(zv, dtype, rows, nlist, dim):
    cent, x, ignore = U.label_batch_case(rows, nlist, dim, _npdt(dtype))
    labs = _gpu_labels(zv, cent, x, "SquaredEuclidean", dtype)
    # the reference on both sides of row 2^18 (and the head of the first batch): 4096 rows before the edge, everything after it
    for lo, hi in ((0, 2048), (BATCH - 4096, rows)):
        _check_both(cent, x[lo:hi], "SquaredEuclidean", [l[lo:hi] for l in labs], ignore, "%s rows %d..%d of %d" % (dtype, lo, hi, rows))
    for lab in labs:                                                  # every row was written, with a real centroid
        assert ((lab >= 0) & (lab < nlist)).all() and (lab != nlist - 1).all()
    # and every 61st row of the whole call (rows of every work item position), so that the inside of the full batch is held too
    _check_both(cent, x[::61], "SquaredEuclidean", [l[::61] for l in labs], ignore, "%s every 61st row of %d" % (dtype, rows))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_rows_with_a_common_offset(zv, oracle, dtype):
    """The kernels select on |x|^2 + |c|^2 - 2 x.c; with a common offset the three terms are ~offset^2 dim and cancel to a distance
    of ~dim, and labelling has no direct re-score to fall back on.  The band grows with |x|^2, so only the acceptance rule is
    asserted.  Printed, not asserted (no measurement to take a threshold from; recorded in DESIGN.md, numerics): the share of rows
    labelled differently from the fp64 arg-min and the within-cluster SSE relative to the fp64 labels' — for the GPU and for the
    oracle's direct fp32 sums, which shows how much of the loss is the norm expansion and how much fp32 itself."""
    i = None
    for offset in (0, 10, 100):
        cent, x = U.label_offset_case(offset, _npdt(dtype))
        labs = _gpu_labels(zv, cent, x, "SquaredEuclidean", dtype)
        ref = _check_both(cent, x, "SquaredEuclidean", labs, (), "%s offset %d" % (dtype, offset), cap=None)
        s64, arg = ref[0], ref[1]
        i = np.arange(len(arg))
        olab = oracle.ivf_label_and_pack(cent, x)[0].astype(np.int64)
        U.check_labels(cent, x, "SquaredEuclidean", olab, cap=None, what="oracle offset %d" % offset, ref=ref)
        amb = U.label_ambiguous(*ref)
        for name, lab in [("gpu tile %d" % t, l) for t, l in enumerate(labs)] + [("oracle fp32 direct", olab)]:
            print("OFFSET %s offset %3d x spread, %-18s: differs from fp64 arg-min %.4f %% of rows, SSE ratio %.8f (ambiguous rows %.2f %%)"
                  % (dtype, offset, name, 100.0 * (lab != arg).mean(), s64[i, lab].sum() / s64[i, arg].sum(), 100.0 * amb.mean()))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
def test_rows_without_a_finite_score(zv, dtype, metric):
    """One row with a NaN, one with +inf, one with -inf among ordinary rows.  label_dev returns 0 and labels the ordinary rows as
    the reference says.  What the odd rows get is pinned as the code does it:
      NaN row    every score is NaN.  assign_kernel clamps with fmaxf(score, floor), which returns the floor for a NaN: every column
                 scores alike and the first wins -> label 0.  assign256_f16_kernel compares the raw NaN: no comparison is true
                 -> IDX_NONE, which zvec_hip_ivf_label_dev hands to the caller and build / train clamp to list 0 on the host.
      +-inf row  x.c is +-inf by the sign of the centroid's element in that column: the first centroid whose element has the
                 sign of the row's infinity scores lowest (NaN clamped to the floor, or -inf) -> that id, from both kernels."""
    import torch
    n, nlist, dim = 600, 200, 72
    npdt = _npdt(dtype)
    cent, x, ignore = U.label_case(n, nlist, dim, npdt, "means", metric, seed=3)
    odd = {5: (11, np.nan), 301: (3, np.inf), 599: (7, -np.inf)}          # none of them in build()'s strided sample
    for r, (col, v) in odd.items():
        x[r, col] = v
    ordinary = np.setdiff1d(np.arange(n), list(odd))
    labs = _gpu_labels(zv, cent, x, metric, dtype)
    _check_both(cent, x[ordinary], metric, [l[ordinary] for l in labs], ignore, "%s %s ordinary rows" % (dtype, metric))
    for t, lab in enumerate(labs):
        tile256 = dtype == "fp16" and t == 0
        print("non-finite rows, %s %s labels %d: %r" % (dtype, metric, t, [int(lab[r]) for r in odd]))
        for r in odd:
            assert 0 <= lab[r] < nlist or lab[r] == IDX_NONE
        assert lab[5] == (IDX_NONE if tile256 else 0)
        assert lab[301] == np.nonzero(cent[:, 3] > 0)[0][0]
        assert lab[599] == np.nonzero(cent[:, 7] < 0)[0][0]
    # the one-call build of the same rows: no path indexes with an unclamped label (ivf_train and zvec_hip_ivf_build_dev clamp,
    # ivf_pack / ivf_add_rows refuse with InvalidArgument), every row lands in exactly one list.  The sample is rows
    # floor(i * 600 / 192): the odd rows are not in it, so the trained centroids are finite and the rule above places them
    S = 16 * 12
    assert not set((np.arange(S) * n) // S) & set(odd)
    se = zv.HipIVFSearcher(dim, metric, dtype=dtype)
    assert se.build(x, 12, kmeans_iters=2, sample_per_list=16, seed=4) == 0
    c2, offs, order = se.export()
    assert np.isfinite(c2.astype(np.float64)).all()
    assert int(offs[-1]) == n and np.array_equal(np.sort(order), np.arange(n, dtype=np.uint64))
    sizes = np.diff(offs.astype(np.int64))
    assert sizes.sum() == n and (sizes >= 0).all()
    where = np.empty(n, np.int64)
    where[order.astype(np.int64)] = np.repeat(np.arange(12), sizes)
    print("non-finite rows, %s %s build: lists %r" % (dtype, metric, [int(where[r]) for r in odd]))
    assert where[5] == 0                                               # the NaN row: label 0, or IDX_NONE clamped to list 0
    assert where[301] == np.nonzero(c2[:, 3] > 0)[0][0] and where[599] == np.nonzero(c2[:, 7] < 0)[0][0]
    # and a caller that passes label_dev's IDX_NONE on to add_dev is refused, not indexed with
    st = zv.HipIVFSearcher(dim, metric, dtype=dtype)
    assert st.set_centroids(cent) == 0
    assert st.begin_lists(np.bincount(np.zeros(1, np.int64), minlength=nlist)) == 0
    d_row = torch.from_numpy(x[:1]).cuda()
    assert st.add_dev(d_row.data_ptr(), 1, np.array([IDX_NONE], np.uint32), 0) == zv.IndexError_.InvalidArgument


# ---- the k-means step -----------------------------------------------------------------------------------------------------------
def _train(zv, sample, nlist, iters, seed, dtype, metric="SquaredEuclidean"):
    import torch
    se = zv.HipIVFSearcher(sample.shape[1], metric, dtype=dtype)
    d = torch.from_numpy(sample).cuda()
    assert se.train_dev(d.data_ptr(), len(sample), nlist, kmeans_iters=iters, seed=seed) == 0
    torch.cuda.synchronize()
    return se.get_centroids()


def _source_rows(sample, cent):
    """row number of the sample row every centroid is byte-equal to (the sample's rows are distinct)"""
    where = {sample[i].tobytes(): i for i in range(len(sample))}
    assert len(where) == len(sample)
    src = [where.get(cent[l].tobytes(), -1) for l in range(len(cent))]
    assert min(src) >= 0, "a centroid that is no sample row"
    return np.asarray(src)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_initial_centroids_are_distinct_sample_rows_chosen_by_the_seed(zv, dtype):
    S, dim, nlist = 5000, 40, 300
    sample = np.random.default_rng(21).standard_normal((S, dim)).astype(_npdt(dtype))
    c0 = _train(zv, sample, nlist, 0, 17, dtype)
    assert c0.shape == (nlist, dim) and c0.dtype == sample.dtype
    src = _source_rows(sample, c0)
    assert len(set(src.tolist())) == nlist
    assert _train(zv, sample, nlist, 0, 17, dtype).tobytes() == c0.tobytes()         # a fresh handle, the same seed
    other = _source_rows(sample, _train(zv, sample, nlist, 0, 18, dtype))
    assert len(set(other.tolist())) == nlist and not np.array_equal(other, src)
    # the choice depends on the seed and the sample size only, not on what the rows hold
    assert np.array_equal(_source_rows(sample[::-1].copy(), _train(zv, sample[::-1].copy(), nlist, 0, 17, dtype)), src)


def _half_ulp16(v):
    """half an ulp of the half nearest to |v|, with the subnormal floor (exponent -14, 10 fraction bits)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


@pytest.mark.parametrize("dim", [1, 255, 256, 257, 768])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_one_lloyd_round_is_the_fp64_mean_of_the_members(zv, dtype, dim):
    """centroid_mean_kernel (256 threads stride the columns: dims 255 / 256 / 257 are one short of, exactly and one past a pass)
    against the fp64 mean under the labels label_dev gives for the initial codebook: one cluster of > 50 000 members (a mean that
    drifts shows there), clusters of ONE member (a wrong divisor shows there), a cluster of two equal rows, and an empty one —
    a copy of an earlier centroid, which no row prefers — that must keep its initial centroid bit for bit."""
    import torch
    S, nlist, seed = 50200, 8, 29
    npdt = _npdt(dtype)
    # which sample rows the seed picks depends on (seed, S, nlist) only (test above): find them with a probe of row numbers
    picks = _train(zv, np.arange(S, dtype=np.float32)[:, None], nlist, 0, seed, "fp32")[:, 0].astype(np.int64)
    assert len(set(picks.tolist())) == nlist
    rng = np.random.default_rng([31, dim])
    sample = (rng.uniform(1.0, 4.0, dim)[None] + rng.standard_normal((S, dim))).astype(npdt)          # the blob
    for k in range(1, nlist):                                          # far-away rows, each alone ...
        sample[picks[k]] = (100.0 * (k + 1) * rng.choice([-1.0, 1.0], dim) + rng.standard_normal(dim)).astype(npdt)
    sample[picks[2]] = sample[picks[1]]                                # ... but two of them equal: list 2 must stay empty
    c0 = _train(zv, sample, nlist, 0, seed, dtype)
    assert np.array_equal(c0.view(np.uint8), sample[picks].view(np.uint8))
    se = zv.HipIVFSearcher(dim, "SquaredEuclidean", dtype=dtype)
    assert se.set_centroids(c0) == 0
    lab = _label(se, torch.from_numpy(sample).cuda(), S)
    sizes = np.bincount(lab, minlength=nlist)
    assert sizes.sum() == S and sizes.max() >= 50000 and (sizes == 1).sum() >= 3 and sizes[2] == 0 and sizes[1] == 2
    c1 = _train(zv, sample, nlist, 1, seed, dtype)
    worst = 0.0
    for l in range(nlist):
        if sizes[l] == 0:
            assert c1[l].tobytes() == c0[l].tobytes(), "empty list %d lost its centroid" % l
            continue
        mem = sample[lab == l].astype(np.float64)
        m = len(mem)
        mean = mem.mean(0)
        # m terms summed one after the other in fp32: every partial sum is rounded once, so term i meets at most m - i + 1
        # roundings of 2^-24 relative, each of a partial sum no larger than sum|x|: |sum error| <= (m - 1) 2^-24 sum|x|.  The
        # divisor 1 / m is rounded (one more 2^-24), the product acc * inv again: |error of the mean| <= (m + 1) 2^-24 mean|x|
        # to first order; (m + 2) covers the second-order terms of clusters of a few members.
        bound = (m + 2) * 2.0 ** -24 * np.abs(mem).mean(0)
        if dtype == "fp16":                                            # + the RNE rounding of that fp32 value to half
            bound = bound + _half_ulp16(np.abs(mean) + bound)
        err = np.abs(c1[l].astype(np.float64) - mean)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (l, m, int(err.argmax()), float(err.max()), float(bound[err.argmax()]))
        if m == 1 or l == 1:
            assert c1[l].tobytes() == sample[lab == l][0].tobytes()      # the mean of one row (or of equal rows) is the row
    print("lloyd round %s dim %d: sizes %r, worst error / bound %.3f" % (dtype, dim, sizes.tolist(), worst))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_empty_clusters_are_split_and_the_build_stays_sound(zv, dtype):
    """fewer distinct points than lists: the initial codebook holds copies, the first round must leave lists empty and ivf_train
    re-seeds them by splitting the largest cluster"""
    n, dim, nlist = 600, 24, 16
    npdt = _npdt(dtype)
    rng = np.random.default_rng(41)
    points = (5.0 * rng.standard_normal((6, dim))).astype(npdt)
    x = np.ascontiguousarray(points[rng.integers(0, 6, n)])
    cent = _train(zv, x, nlist, 3, 43, dtype)
    assert cent.shape == (nlist, dim) and np.isfinite(cent.astype(np.float64)).all()
    se = zv.HipIVFSearcher(dim, "SquaredEuclidean", dtype=dtype)
    assert se.build(x, nlist, kmeans_iters=3, sample_per_list=64, seed=43) == 0
    c2, offs, order = se.export()
    assert np.isfinite(c2.astype(np.float64)).all()
    sizes = np.diff(offs.astype(np.int64))
    assert sizes.sum() == n and np.array_equal(np.sort(order), np.arange(n, dtype=np.uint64))
    lab = np.empty(n, np.int64)
    lab[order.astype(np.int64)] = np.repeat(np.arange(nlist), sizes)
    s64, arg, gap, E = U.label_reference(c2, x, "SquaredEuclidean")
    assert U.label_accept(s64, arg, E, lab).all()
    assert len(np.unique(c2, axis=0)) > 6                              # the split made new centroids: more than there are points
