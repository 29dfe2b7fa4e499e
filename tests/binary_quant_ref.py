"""Numpy restatement of ailego::BinaryQuantizer::encode as the binary-quantisation tests use it (numpy only; nothing here touches
the GPU or the library).

encode(in, encode_dims, out) written into a zeroed row of ceil(dim / 32) uint32 words: bit i of a row (bit i % 32 of word i // 32,
LSB first) is in[i] >= threshold for i < encode_dims and 0 otherwise.  The comparison is numpy's fp32 `>=`, which is IEEE's: -0.0 >= 0.0
holds, nan compares false, +inf true, -inf false, a denormal compares by its value.
"""
import numpy as np


def converter_encode_dims(dim):
    """what BinaryConverterHolder::Iterator::encode_record passes as the dimension: half of the PADDED bit count"""
    return (int(dim) + 31) // 32 * 32 // 2


def binary_encode_reference(rows, threshold=0.0, encode_dims=None):
    """rows: [count][dim] fp32 -> uint32 [count][ceil(dim / 32)]"""
    rows = np.asarray(rows, np.float32)
    assert rows.ndim == 2
    count, dim = rows.shape
    encode_dims = dim if encode_dims is None else int(encode_dims)
    assert 1 <= encode_dims <= dim
    words = (dim + 31) // 32
    bits = np.zeros((count, words * 32), np.uint8)
    with np.errstate(invalid="ignore"):
        bits[:, :encode_dims] = rows[:, :encode_dims] >= np.float32(threshold)
    weights = np.uint32(1) << np.arange(32, dtype=np.uint32)
    return (bits.reshape(count, words, 32).astype(np.uint32) * weights).sum(axis=2, dtype=np.uint32)
