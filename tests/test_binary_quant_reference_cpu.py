"""CPU checks of the binary-quantisation feature: the numpy restatement of BinaryQuantizer::encode (tests/binary_quant_ref.py)
against answers written out by hand, and the C example against the header.

The reference's own converted rows are NOT among the sources: through the existing doors of oracle/refcore.py,
build_converted("FlatBuilder", "BinaryConverter", ...) reaches BinaryConverter, whose `quantizer_` member is never created
(binary_converter.cc:138-167, :223), so the first encode_record dereferences a null pointer; and BinaryReformer is reachable only
through an index that converter has built.  No door was added for either."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binary_quant_ref import binary_encode_reference, converter_encode_dims  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENORMAL = np.float32(1e-40)
assert 0 < DENORMAL < np.finfo(np.float32).tiny


def test_special_values_at_threshold_zero():
    row = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, DENORMAL, -DENORMAL, 1.0, -1.0]], np.float32)
    #                1     1     0       1       0        1         0          1     0    -> bits 0, 1, 3, 5, 7
    assert binary_encode_reference(row).tolist() == [[0b010101011]]


def test_nonzero_thresholds():
    row = np.array([[0.25, 0.2499, 0.5, -1.0, -0.75, -1.5, np.nan, np.inf]], np.float32)
    assert binary_encode_reference(row, 0.25).tolist() == [[0b10000101]]
    assert binary_encode_reference(row, -1.0).tolist() == [[0b10011111]]
    # a denormal threshold separates denormals: nothing is flushed to zero
    row = np.array([[0.0, DENORMAL, 2 * DENORMAL, -DENORMAL]], np.float32)
    assert binary_encode_reference(row, float(DENORMAL)).tolist() == [[0b0110]]
    assert binary_encode_reference(row, float(-DENORMAL)).tolist() == [[0b1111]]


@pytest.mark.parametrize("dim", [1, 31, 32, 33, 63, 64, 65])
def test_all_ones_rows_at_every_width(dim):
    """every value passes: exactly the first encode_dims bits are set, LSB first, and the tail of the last word stays 0"""
    row = np.ones((2, dim), np.float32)
    words = (dim + 31) // 32
    for ed in sorted({1, 31, 32, 33, 63, 64, 65, dim}):
        if ed > dim:
            continue
        got = binary_encode_reference(row, 0.0, ed)
        assert got.shape == (2, words) and got.dtype == np.uint32
        want = [(((1 << ed) - 1) >> (32 * w)) & 0xffffffff for w in range(words)]
        assert got[0].tolist() == want and got[1].tolist() == want


def test_single_bits_land_lsb_first():
    for dim in (33, 64, 65):
        for i in (0, 1, 30, 31, 32, dim - 1):
            row = np.full((1, dim), -1.0, np.float32)
            row[0, i] = 1.0
            got = binary_encode_reference(row)
            want = [0] * ((dim + 31) // 32)
            want[i // 32] = 1 << (i % 32)
            assert got[0].tolist() == want
            if i >= 1:                                   # a bit at or beyond encode_dims is dropped
                assert not binary_encode_reference(row, 0.0, i).any()


def test_converter_encodes_half_of_the_padded_width():
    assert [converter_encode_dims(d) for d in (1, 31, 32, 33, 63, 64, 65, 768, 1000)] == [16, 16, 16, 32, 32, 32, 48, 384, 512]
    row = np.ones((1, 100), np.float32)
    assert binary_encode_reference(row, 0.0, converter_encode_dims(100)).tolist() == [[0xffffffff, 0xffffffff, 0, 0]]


def test_rows_are_independent():
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((5, 70)).astype(np.float32)
    both = binary_encode_reference(rows, 0.1, 66)
    for i in range(5):
        assert np.array_equal(both[i:i + 1], binary_encode_reference(rows[i:i + 1], 0.1, 66))
    bits = np.unpackbits(both.view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(bits[:, :66].astype(bool), rows[:, :66] >= np.float32(0.1)) and not bits[:, 66:].any()


def test_c_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "binary_quantize")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "binary_quantize.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        assert os.path.exists(exe)
