"""The fp64 labelling reference of tests/util.py and its derived band, before a GPU sees them: the oracle's restatement of
IVFBuilder::label (fp32 / fp16 rows, direct sums, fp32 accumulation) labels what the generators of tests/test_gpu_label_parity.py
give (the same seeded cases; of the batch-edge rows the first blocks); its labels must pass the acceptance rule (the band is not
too tight for a correct fp32 implementation), at most 1 % of the rows may be ambiguous, a quarter of the rows sits 3-30 bands
from a bisector, and scores with the error of a half-precision accumulation are REJECTED on those rows (the band decides
something).  Also what the band claims against test_gpu_build.py's former hand-picked one."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util as U

METRICS = {"SquaredEuclidean": O.METRIC_L2, "InnerProduct": O.METRIC_IP}


def test_reference_on_a_case_worked_by_hand():
    cent = np.array([[0, 0], [3, 0], [0, 0], [0, 4]], np.float32)
    rows = np.array([[1, 0], [2, 0], [1.5, 0], [0, 3]], np.float32)
    s64, arg, gap, E = U.label_reference(cent, rows, "SquaredEuclidean", ignore=(2,))
    assert np.array_equal(s64, [[1, 4, 1, 17], [4, 1, 4, 20], [2.25, 2.25, 2.25, 18.25], [9, 18, 9, 1]])
    assert np.array_equal(arg, [0, 1, 0, 3])                       # the exact tie of row 2 goes to the first
    assert np.array_equal(gap, [3, 3, 0, 8])
    g = (32 + 8) * 2.0 ** -23
    assert np.allclose(E[0], g * np.array([1, 16, 1, 25.0]), rtol=1e-15)
    assert np.array_equal(U.label_ambiguous(s64, arg, gap, E, (2,)), [False, False, True, False])
    assert np.array_equal(U.label_accept(s64, arg, E, [0, 1, 1, 3]), [True] * 4)
    assert np.array_equal(U.label_accept(s64, arg, E, [1, 1, 0, 0xffffffff]), [False, True, True, False])
    s, a, _, e = U.label_reference(cent, rows, "InnerProduct")
    assert np.array_equal(s[:, 1], [-3, -6, -4.5, 0]) and np.array_equal(a, [1, 1, 1, 3])
    assert np.allclose(e[:, 1], g * np.array([3, 6, 4.5, 0]), rtol=1e-15)
    with pytest.raises(AssertionError):
        U.check_labels(cent, rows, "SquaredEuclidean", [0, 0, 0, 3], ignore=(2,), cap=None)      # row 1 is plainly wrong
    with pytest.raises(AssertionError):
        U.check_labels(cent, rows, "SquaredEuclidean", [0, 1, 2, 3], ignore=(2,), cap=None)      # the duplicate id
    assert U.label_scan_width(100, np.float16) == (100, 128) and U.label_scan_width(33, np.float32, "Cosine") == (32, 32)


def _narrowed_labels(ref, dpad, ignore):
    """labels of a kernel that accumulates with 11 significant bits: every score off by up to 2^-11 of the magnitudes summed
    ((|x| + |c|)^2, sum|x_i||c_i|), which is E with 2^-11 in place of gamma"""
    s64, _, _, E = ref
    s = s64 + E * (2.0 ** -11 / ((dpad + 8) * 2.0 ** -23)) * np.random.default_rng(1).uniform(-1, 1, s64.shape)
    if len(ignore):
        s[:, list(ignore)] = np.inf
    return s.argmin(1)


@pytest.mark.parametrize("dtype,kind", U.LABEL_KINDS)
def test_oracle_labels_pass_the_band_and_inputs_are_unambiguous(oracle, dtype, kind):
    """Per shape and metric: the oracle's fp32 labels pass every check the GPU labels meet; a quarter of the rows is decided by
    the band (3-30 bands from a bisector, none of them ambiguous); and labels from scores with a half-precision accumulation
    error fail the acceptance rule.  That last check stops at a scan width of 256: gamma = (d_pad + 8) 2^-23 grows with the
    width and at 768 dims is 2^-13.4, within 5x of half precision, less than the 6 bands the near rows keep clear."""
    npdt = np.float16 if dtype == "fp16" else np.float32
    for rows, nlist, dim in U.LABEL_SHAPES:
        for metric, mid in METRICS.items():
            what = "%s %s %s %r" % (dtype, kind, metric, (rows, nlist, dim))
            cent, x, ignore = U.label_case(rows, nlist, dim, npdt, kind, metric)
            lab, _, _ = oracle.ivf_label_and_pack(cent, x, mid)
            ref = U.check_labels(cent, x, metric, lab, ignore, what="oracle " + what)
            if nlist < 2:
                continue
            assert U.label_near_share(*ref, ignore) >= 0.2, what
            dpad = U.label_scan_width(dim, npdt, metric)[1]
            if dpad <= 256:
                narrow = _narrowed_labels(ref, dpad, ignore)
                assert (~U.label_accept(ref[0], ref[1], ref[3], narrow)).sum() >= 3, what
                with pytest.raises(AssertionError):
                    U.check_labels(cent, x, metric, narrow, ignore, what=what, ref=ref)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_cosine_inputs_are_unambiguous(dtype):
    npdt = np.float16 if dtype == "fp16" else np.float32
    for rows, nlist, dim in U.LABEL_SHAPES:
        if dim < 31:
            continue
        cent, x, ignore = U.label_case(rows, nlist, dim, npdt, "means", "Cosine")
        s64, arg, gap, E = U.label_reference(cent, x, "Cosine", ignore)
        assert U.label_ambiguous(s64, arg, gap, E, ignore).sum() <= 0.01 * rows
        assert U.label_near_share(s64, arg, gap, E, ignore) >= 0.2
        assert s64.shape == (rows, nlist) and (np.abs(1 - s64) <= 1 + 1e-2).all()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("offset", [0, 10, 100])
def test_oracle_labels_pass_the_band_with_a_common_offset(oracle, dtype, offset):
    npdt = np.float16 if dtype == "fp16" else np.float32
    cent, x = U.label_offset_case(offset, npdt)
    lab, _, _ = oracle.ivf_label_and_pack(cent, x)
    U.check_labels(cent, x, "SquaredEuclidean", lab, cap=None, what="oracle offset %d %s" % (offset, dtype))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_batch_edge_inputs_are_unambiguous(oracle, dtype):
    npdt = np.float16 if dtype == "fp16" else np.float32
    cent, x, ignore = U.label_batch_case(3 * 4096 + 300, 200, 72, npdt)          # the first blocks of what the GPU case labels
    assert np.array_equal(x[:4096 + 7], U.label_batch_case(4096 + 7, 200, 72, npdt)[1])
    assert len(np.unique(x, axis=0)) == len(x)
    lab, _, _ = oracle.ivf_label_and_pack(cent, x)
    ref = U.check_labels(cent, x, "SquaredEuclidean", lab, ignore, what="oracle batch rows %s" % dtype)
    assert U.label_near_share(*ref, ignore) >= 0.2


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_derived_band_against_the_former_hand_picked_one(dtype):
    """test_labelling_and_packing_integer_data_exact compared scores within 4e-6 (|x|^2 + |c|^2) and allowed n // 1000 rows to
    differ.  On that data (integers in [-8, 8], 48 dims, centroids = means of ~300 rows) the derived band E(x, g) + E(x, argmin)
    = 2 (64 + 8) 2^-23 (|x| + |c|)^2 is WIDER than the hand-picked one, so the GPU test keeps the old band and adds the derived
    checks; the count of ambiguous rows, on the other hand, is far below n // 1000."""
    npdt = np.float16 if dtype == "fp16" else np.float32
    rng = np.random.default_rng(11)
    n, dim, nlist = 20000, 48, 64
    base = rng.integers(-8, 9, (n, dim)).astype(npdt)
    cent = base[(np.arange(64 * nlist) * n) // (64 * nlist)][:nlist].astype(np.float64)
    for _ in range(3):                                              # three Lloyd rounds in fp64 stand in for the GPU's
        lab = ((base.astype(np.float64) ** 2).sum(1)[:, None] + (cent ** 2).sum(1)[None] - 2 * base.astype(np.float64) @ cent.T).argmin(1)
        for l in range(nlist):
            if (lab == l).any():
                cent[l] = base[lab == l].astype(np.float64).mean(0)
    cent = cent.astype(npdt)
    s64, arg, gap, E = U.label_reference(cent, base, "SquaredEuclidean")
    i = np.arange(n)
    old = 4e-6 * ((base.astype(np.float64) ** 2).sum(1) + (cent.astype(np.float64) ** 2).sum(1)[arg])
    new = 2 * E[i, arg]
    print("derived band / hand-picked band: %.2f .. %.2f; ambiguous rows %d (old cap %d)"
          % ((new / old).min(), (new / old).max(), U.label_ambiguous(s64, arg, gap, E).sum(), n // 1000))
    assert (new > old).all()
    assert U.label_ambiguous(s64, arg, gap, E).sum() <= n // 1000
