"""Verified bf16 MFMA GEMM: numpy reference operands/product and the
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


def reference_product(seed, m, n, k):
    """Exact C[m, n] = A @ B of the generator operands as float32. The
    float64 matmul is exact for these integers (|sum| <= 2^23 << 2^53) and
    BLAS-fast, unlike an int64 matmul."""
    if k > ops.GEMM_EXACT_MAX_K:
        raise ValueError("exact only for K <= 32768")
    a = reference_operand(0, seed, m, k).astype(np.float64)
    b = reference_operand(1, seed, k, n).astype(np.float64)
    return (a @ b).astype(np.float32)


def locate(index, n, where):
    """Map a report element index (m*N + n) to (row, col, tile, xcc, hw_id)
    using the `where` table of the run. XCC id is the low 4 bits of the
    XCC_ID register; hw_id is the raw HW_ID register."""
    row, col = divmod(int(index), int(n))
    tile = (row // ops.GEMM_TILE_M) * (int(n) // ops.GEMM_TILE_N) \
        + col // ops.GEMM_TILE_N
    return (row, col, tile, int(where[tile][0]) & 0xF,
            int(where[tile][1]) & 0xFFFFFFFF)


def gemmtest(m, n, k, iters=1, seed=0, device="cuda:0", gold_hook=None):
    """Run the compute-integrity test; returns (MemReport, flops, where).

    Fill A and Bt from the generator, compute gold once with the integer
    VALU kernel, then `iters` times: MFMA GEMM -> bitwise compare against
    gold. Everything is queued on the current stream; the only host sync
    is the final report read. Report indices are element indices m*N + n;
    `where` is the int32[tiles, 2] host array of the last GEMM (see
    ``locate``). `gold_hook(gold)` runs once on the gold tensor before the
    loop — the drill hook for exercising the miscompare path.
    """
    import torch

    a = torch.empty((m, k), dtype=torch.bfloat16, device=device)
    bt = torch.empty((n, k), dtype=torch.bfloat16, device=device)
    ops.gemm_fill(a, 0, seed, m, k)
    ops.gemm_fill(bt, 1, seed, n, k)
    return _verify_loop((a, bt), ops.gemm_ref_int, ops.gemm_bf16_nt, m, n, k,
                        iters, gold_hook)


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
