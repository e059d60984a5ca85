"""Verified dense MFMA GEMM (bf16 and the fp16 / int8 / fp32 / fp64
formats): numpy reference operands/product and the
compute-integrity driver.

``reference_operand`` is an independent re-implementation of
``hip/gemm_pattern.h`` in numpy integer arithmetic — the oracle the fill
kernel and ``mi-stream --gemm-operand-dump`` are tested against.
``reference_product`` is the exact product of those operands.

Operands are integers in [-16, 15], so |a*b| <= 256 and a length-K sum is
at most 256*K in magnitude: for K <= 32768 that is <= 2^23, every partial
sum in any order is an integer fp32 holds exactly, and the correct C is
unique. ``gemmtest`` therefore compares the matrix-pipe result bitwise
against a gold computed once by the integer VALU kernel.

The other dense formats (``fmt`` = fp16, int8, fp32, fp64; see
``ops.GEMM_FORMATS``) take the same operands. fp16 and fp32 inherit the
argument above unchanged: the operands have at most 5 significant bits,
which both formats hold, and accumulation is fp32, so |sum| <= 256*K <=
2^23 is exact. int8 accumulates in int32 and fp64 in fp64, exact up to
2^31 and 2^53: far beyond the cap, which stays K <= 32768 for every format.
The comparison is bitwise in every format.
"""

from __future__ import annotations

import numpy as np

from k3samd import ops

_M32 = np.uint64(0xFFFFFFFF)


def _mul32(a, b):
    return (a * np.uint64(b)) & _M32


def reference_operand(which, seed, rows, cols, row0=0, col0=0):
    """Logical operand window as int32[rows, cols]: element [i][j] is
    gemm_operand(seed, which, row0 + i, col0 + j); which = 0 is A[m][k],
    which = 1 is B[k][n]. Values are carried in uint64 and masked to 32
    bits after every multiply, so nothing depends on numpy's wrap-around.
    """
    if which not in (0, 1):
        raise ValueError("which must be 0 (A) or 1 (B)")
    seed = int(seed) & ((1 << 64) - 1)
    r = (np.uint64(row0) + np.arange(rows, dtype=np.uint64))[:, None] & _M32
    c = (np.uint64(col0) + np.arange(cols, dtype=np.uint64))[None, :] & _M32
    x = _mul32(r, 0x9E3779B1) ^ _mul32(c, 0x85EBCA6B)
    x = x ^ np.uint64(seed & 0xFFFFFFFF)
    x = x ^ _mul32(np.uint64(seed >> 32), 0xC2B2AE35)
    if which:
        x = x ^ np.uint64(0xA5A5A5A5)
    h = x
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> np.uint64(15))
    h = _mul32(h, 0x846CA68B)
    h = h ^ (h >> np.uint64(16))
    return (h >> np.uint64(27)).astype(np.int32) - 16


def _np_result_dtype(fmt):
    if fmt not in ("bf16", "fp16", "int8", "fp32", "fp64"):
        raise ValueError(f"unknown GEMM format {fmt!r}")
    return {"int8": np.int32, "fp64": np.float64}.get(fmt, np.float32)


def reference_product(seed, m, n, k, fmt="bf16"):
    """Exact C[m, n] = A @ B of the generator operands in the result dtype
    of `fmt` (float32, or int32 for int8 and float64 for fp64). The float64
    matmul is exact for these integers (|sum| <= 2^23 << 2^53) and
    BLAS-fast, unlike an int64 matmul."""
    dtype = _np_result_dtype(fmt)
    if k > ops.GEMM_EXACT_MAX_K:
        raise ValueError("exact only for K <= 32768")
    a = reference_operand(0, seed, m, k).astype(np.float64)
    b = reference_operand(1, seed, k, n).astype(np.float64)
    return (a @ b).astype(dtype)


def locate(index, n, where, elem_dwords=1):
    """Map a report dword index to (row, col, tile, xcc, hw_id) using the
    `where` table of the run. With 32-bit results the index is the element
    index m*N + n; with float64 results (`elem_dwords` = 2) it is
    2 * element + half, half 0 being the low dword. XCC id is the low 4
    bits of the XCC_ID register; hw_id is the raw HW_ID register."""
    row, col = divmod(int(index) // int(elem_dwords), int(n))
    tile = (row // ops.GEMM_TILE_M) * (int(n) // ops.GEMM_TILE_N) \
        + col // ops.GEMM_TILE_N
    return (row, col, tile, int(where[tile][0]) & 0xF,
            int(where[tile][1]) & 0xFFFFFFFF)


def gemmtest(m, n, k, iters=1, seed=0, device="cuda:0", gold_hook=None,
             fmt="bf16"):
    """Run the compute-integrity test; returns (MemReport, flops, where).

    Fill A and Bt from the generator in the operand dtype of `fmt`, compute
    gold once with the integer VALU kernel, then `iters` times: MFMA GEMM ->
    bitwise compare against gold. Everything is queued on the current
    stream; the only host sync is the final report read. Report indices are
    element indices m*N + n (for fp64: 2 * element + half); `where` is the
    int32[tiles, 2] host array of the last GEMM (see ``locate``).
    `gold_hook(gold)` runs once on the gold tensor before the loop — the
    drill hook for exercising the miscompare path.
    """
    import torch

    _np_result_dtype(fmt)
    a = torch.empty((m, k), dtype=ops.GEMM_FORMATS[fmt][0], device=device)
    bt = torch.empty((n, k), dtype=ops.GEMM_FORMATS[fmt][0], device=device)
    ops.gemm_fill(a, 0, seed, m, k)
    ops.gemm_fill(bt, 1, seed, n, k)
    if fmt == "bf16":
        ref, gemm = ops.gemm_ref_int, ops.gemm_bf16_nt
    else:
        ref, gemm = ops.gemm_dense_ref_int, ops.gemm_dense_nt
    return _verify_loop((a, bt), ref, gemm, m, n, k, iters, gold_hook)


def _verify_loop(operands, ref, gemm, m, n, k, iters, gold_hook):
    """The tail gemmtest and mxgemmtest share: gold = ref(*operands), the
    hook, then `iters` times gemm(*operands, out=c, where=where) -> bitwise
    compare against gold."""
    import torch

    gold = ref(*operands)
    if gold_hook is not None:
        gold_hook(gold)
    c = torch.empty_like(gold)
    tiles = (m // ops.GEMM_TILE_M) * (n // ops.GEMM_TILE_N)
    where = torch.full((tiles, 2), -1, dtype=torch.int32, device=gold.device)
    report = ops.mem_report_new(gold.device)
    for _ in range(int(iters)):
        gemm(*operands, out=c, where=where)
        ops.buf_compare(c, gold, report)
    rep = ops.mem_report_read(report)
    return rep, 2.0 * m * n * k * int(iters), where.cpu().numpy()
