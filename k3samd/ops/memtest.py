"""HBM pattern memory test: numpy reference pattern and the march driver.

``reference_pattern`` is an independent re-implementation of
``hip/memtest_pattern.h`` in numpy integer arithmetic — the oracle the
kernels and ``mi-stream --memtest-pattern-dump`` are tested against.

``memtest`` runs the moving-inversions march with the HIP kernels. It
covers only the buffer it is given (memory held by anything else is not
touched), and a buffer far larger than the 256 MiB Infinity Cache is needed
for the verify passes to read HBM rather than cache.
"""

from __future__ import annotations

import numpy as np

from k3samd import ops

ADDR = ops.MEM_PATTERN_ADDR
WALK = ops.MEM_PATTERN_WALK
CHECKER = ops.MEM_PATTERN_CHECKER

_M32 = np.uint64(0xFFFFFFFF)


def _rotl32(v, r):
    return ((v << np.uint64(r)) | (v >> np.uint64(32 - r))) & _M32


def reference_pattern(pattern, seed, invert, n_cells, cell_offset=0):
    """Expected memory content as uint32[n_cells, 4] (row = 16-byte cell).

    All values are carried in uint64 and masked to 32 bits after every
    step that can overflow, so nothing depends on numpy's wrap-around.
    """
    seed = int(seed) & ((1 << 64) - 1)
    c = (np.uint64(int(cell_offset) & ((1 << 64) - 1))
         + np.arange(n_cells, dtype=np.uint64))
    c_lo, c_hi = c & _M32, c >> np.uint64(32)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    out = np.empty((n_cells, 4), dtype=np.uint64)
    if pattern == ADDR:
        h = c_lo ^ ((c_hi * np.uint64(0x9E3779B1)) & _M32) ^ s_lo
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x7FEB352D)) & _M32
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x846CA68B)) & _M32
        h ^= h >> np.uint64(16)
        out[:, 0] = h
        out[:, 1] = ~h & _M32
        out[:, 2] = _rotl32(h, 13) ^ c_lo
        out[:, 3] = _rotl32(h, 7) ^ c_hi ^ s_hi
    elif pattern == WALK:
        for k in range(4):
            g_lo = (c_lo * np.uint64(4) + np.uint64(k)) & _M32
            out[:, k] = np.uint64(1) << ((g_lo + s_lo) & np.uint64(31))
    elif pattern == CHECKER:
        for k in range(4):
            odd = (c_lo + np.uint64(k) + s_lo) & np.uint64(1)
            out[:, k] = np.where(odd == 1, np.uint64(0x55555555),
                                 np.uint64(0xAAAAAAAA))
    else:
        raise ValueError(f"unknown memtest pattern id {pattern}")
    if invert:
        out = ~out & _M32
    return out.astype(np.uint32)


def memtest(buf, passes=1, seed=0):
    """Run the march on `buf`; returns (MemReport, bytes_moved).

    Per pass p, with s = seed + p:
      fill(ADDR) -> verify_fill(ADDR -> ~ADDR) -> verify_fill(~ADDR -> WALK)
      -> verify_fill(WALK -> CHECKER) -> verify(CHECKER)
    i.e. 8 buffer-sized transfers. Everything is queued on the current
    stream; the only host sync is the final report read.
    """
    report = ops.mem_report_new(buf.device)
    nbytes = buf.numel() * buf.element_size()
    moved = 0
    for p in range(int(passes)):
        s = (int(seed) + p) & ((1 << 64) - 1)
        ops.mem_fill(buf, ADDR, s)
        ops.mem_verify_fill(buf, report, (ADDR, s, False), (ADDR, s, True))
        ops.mem_verify_fill(buf, report, (ADDR, s, True), (WALK, s, False))
        ops.mem_verify_fill(buf, report, (WALK, s, False),
                            (CHECKER, s, False))
        ops.mem_verify(buf, report, CHECKER, s)
        moved += 8 * nbytes
    return ops.mem_report_read(report), moved
