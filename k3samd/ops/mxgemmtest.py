"""Verified MX (block-scaled fp8 e4m3 / fp4 e2m1) MFMA GEMM: numpy reference
operands, scales and product, and the compute-integrity driver.

``reference_elements`` and ``reference_scales`` are an independent
re-implementation of ``hip/mx_pattern.h`` in numpy: the hash in masked
uint64 arithmetic, the fp8 byte by inverting a decode table of all 256
e4m3fn codes (the header encodes with shifts), the fp4 value by table
lookup. They are the oracle the fill kernel and ``mi-mxgemm``'s dumps are
tested against. ``reference_product`` is the exact product of the scaled
operands.

Exactness: a scaled fp8 element is an integer with |v| <= 16 * 2 = 32, so
|a*b| <= 1024 and a length-K sum is at most 1024*K <= 2^23 for K <= 8192. A
scaled fp4 element is at most 6 * 2 = 12 = 24 halves, a product at most 576
quarters, and 576 * 8192 < 2^23 quarters. Every partial sum in any order is
held exactly by fp32, the correct C is unique, and ``mxgemmtest`` compares
the matrix-pipe result bitwise against a gold computed once by the integer
VALU kernel.
"""

from __future__ import annotations

import numpy as np

from k3samd import ops
from k3samd.ops.gemmtest import _verify_loop
from k3samd.ops.gemmtest import locate  # noqa: F401  (same tile geometry)

_M32 = np.uint64(0xFFFFFFFF)
_SCALE_SALT = 0x3C6EF372

FP4_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                       -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


def _e4m3_table():
    """float64 value of every e4m3fn byte (0x7F and 0xFF are NaN)."""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6,
                   (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))
    mag[(b & 0x7F) == 0x7F] = np.nan
    return np.where(b & 0x80, -mag, mag)


E4M3_VALUES = _e4m3_table()
# byte of each integer -16..15 (index v + 16), found in the decode table
_E4M3_OF_INT = np.array(
    [int(np.flatnonzero(E4M3_VALUES == v)[0]) for v in range(-16, 16)],
    dtype=np.uint8)


def _mul32(a, b):
    return (a * np.uint64(b)) & _M32


def _hash(which, seed, r, c, salt=0):
    """lowbias32 over (r, c, seed, which, salt), uint64 arrays masked to 32
    bits after every multiply."""
    if which not in (0, 1):
        raise ValueError("which must be 0 (A) or 1 (B)")
    seed = int(seed) & ((1 << 64) - 1)
    x = _mul32(r & _M32, 0x9E3779B1) ^ _mul32(c & _M32, 0x85EBCA6B)
    x = x ^ np.uint64(seed & 0xFFFFFFFF)
    x = x ^ _mul32(np.uint64(seed >> 32), 0xC2B2AE35)
    if which:
        x = x ^ np.uint64(0xA5A5A5A5)
    h = x ^ np.uint64(salt)
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> np.uint64(15))
    h = _mul32(h, 0x846CA68B)
    return h ^ (h >> np.uint64(16))


def _window(rows, cols, row0, col0):
    r = (np.uint64(row0) + np.arange(rows, dtype=np.uint64))[:, None]
    c = (np.uint64(col0) + np.arange(cols, dtype=np.uint64))[None, :]
    return r, c


def _check_fmt(fmt):
    if fmt not in (ops.MX_FMT_FP8, ops.MX_FMT_FP4):
        raise ValueError("fmt must be 0 (fp8 e4m3) or 4 (fp4 e2m1)")


def reference_elements(fmt, which, seed, rows, cols, row0=0, col0=0):
    """Logical operand window: (float64 values, uint8 raw codes), each
    [rows, cols]; element [i][j] is at (row0 + i, col0 + j); which = 0 is
    A[m][k], which = 1 is B[k][n]. Unscaled."""
    _check_fmt(fmt)
    h = _hash(which, seed, *_window(rows, cols, row0, col0))
    if fmt == ops.MX_FMT_FP8:
        codes = _E4M3_OF_INT[(h >> np.uint64(27)).astype(np.int64)]
        return E4M3_VALUES[codes], codes
    codes = (h >> np.uint64(28)).astype(np.uint8)
    return FP4_VALUES[codes], codes


def reference_scales(which, seed, rows, blocks, row0=0, blk0=0):
    """E8M0 bytes uint8[rows, blocks] of stored rows row0.. (m of A for
    which = 0, n of Bt for which = 1) and k-blocks blk0.. of 32 k."""
    h = _hash(which, seed, *_window(rows, blocks, row0, blk0),
              salt=_SCALE_SALT)
    return (np.uint64(127) + (h >> np.uint64(31))).astype(np.uint8)


def pack_codes(fmt, codes):
    """Raw codes [rows, k] -> stored bytes: [rows, k] for fp8, [rows, k/2]
    for fp4 with the even k in the low nibble."""
    _check_fmt(fmt)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if fmt == ops.MX_FMT_FP8:
        return codes
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def scaled_operands(fmt, seed, m, n, k):
    """float64 (A∘SA)[m, k] and (B∘SB)[k, n] of the generator."""
    if k % 32:
        raise ValueError("k must be a multiple of 32")
    a, _ = reference_elements(fmt, 0, seed, m, k)
    b, _ = reference_elements(fmt, 1, seed, k, n)
    sa = reference_scales(0, seed, m, k // 32).astype(np.float64) - 127
    sb = reference_scales(1, seed, n, k // 32).astype(np.float64) - 127
    return (a * np.repeat(2.0 ** sa, 32, axis=1),
            b * np.repeat(2.0 ** sb, 32, axis=1).T)


def reference_product(fmt, seed, m, n, k):
    """Exact C[m, n] = (A∘SA) @ (B∘SB) of the generator as float32. The
    float64 matmul is exact: every term is a multiple of 1/4 and every sum
    stays below 2^23 of them."""
    if k > ops.MX_EXACT_MAX_K:
        raise ValueError("exact only for K <= 8192")
    a, b = scaled_operands(fmt, seed, m, n, k)
    return (a @ b).astype(np.float32)


def mxgemmtest(m, n, k, fmt, iters=1, seed=0, device="cuda:0",
               gold_hook=None):
    """Run the MX compute-integrity test; returns (MemReport, flops, where).

    Fill A, SA, Bt and SB from the generator, compute gold once with the
    integer VALU kernel, then `iters` times: block-scaled MFMA GEMM ->
    bitwise compare against gold. Everything is queued on the current
    stream; the only host sync is the final report read. Report indices,
    `where` and `gold_hook` are as in ``gemmtest.gemmtest``; ``locate``
    maps an index to its tile.
    """
    import torch

    _check_fmt(fmt)
    kb = k // 2 if fmt == ops.MX_FMT_FP4 else k
    a = torch.empty((m, kb), dtype=torch.uint8, device=device)
    bt = torch.empty((n, kb), dtype=torch.uint8, device=device)
    sa = torch.empty((m, k // 32), dtype=torch.uint8, device=device)
    sb = torch.empty((n, k // 32), dtype=torch.uint8, device=device)
    ops.mx_fill(a, sa, 0, seed, m, k, fmt)
    ops.mx_fill(bt, sb, 1, seed, n, k, fmt)
    return _verify_loop((a, sa, bt, sb, fmt), ops.mx_gemm_ref_int,
                        ops.mx_gemm_nt, m, n, k, iters, gold_hook)
