"""HBM memory-test kernels on the GPU: fill / verify / verify-fill against
the numpy reference pattern, exact accounting of planted corruption, the
64-bit offset path, the march driver and the mi-stream --memtest binary.

Sizes are the smallest at which the kernels can still go wrong: one cell,
either side of a wave (64) and of a block (256), several blocks with a
ragged tail (785), and many blocks (65536)."""

import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops.memtest import (ADDR, CHECKER, WALK, memtest,
                                reference_pattern)

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_STREAM = REPO / "native" / "bin" / "mi-stream"

SIZES = [1, 63, 64, 65, 255, 256, 257, 785, 65536]
PATTERNS = [ADDR, WALK, CHECKER]
SEED = 0xDEADBEEF12345678
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def ref(pattern, seed, invert, n_cells, cell_offset=0):
    """Reference computed once per case and shared; returned read-only."""
    r = reference_pattern(pattern, seed, invert, n_cells, cell_offset)
    r.setflags(write=False)
    return r


def new_buf(n_cells):
    # poison so that a cell the kernel skipped cannot match by accident
    return torch.full((n_cells * 4,), 0x5A5A5A5A, dtype=torch.int32,
                      device=DEV)


def cells(buf):
    return buf.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 4)


def plant(buf, flips):
    """XOR mask into dword g for every (g, mask) with torch indexing."""
    idx = torch.tensor([g for g, _ in flips], dtype=torch.int64, device=DEV)
    masks = np.array([m for _, m in flips], dtype=np.uint32).view(np.int32)
    flat = buf.view(torch.int32)
    flat[idx] = flat[idx] ^ torch.from_numpy(masks).to(DEV)


def standard_flips(n_cells):
    """Dword 0, the last dword, dword 1 of the last cell (in the final
    partial wave for n_cells = 65 and 257) and one in the middle."""
    flips = {0: 0x00000001, 4 * n_cells - 1: 0x80000000,
             4 * (n_cells // 2) + 2: 0x00010100}
    if n_cells > 1:
        flips[4 * (n_cells - 1) + 1] = 0xFFFFFFFF
    return sorted(flips.items())


def many_flips(n_cells, count=40):
    """`count` distinct dwords spread over the region, first and last
    included, with varied masks."""
    last = 4 * n_cells - 1
    gs = sorted({0, last} | {(i * last) // (count - 1) for i in range(count)})
    assert len(gs) == count
    return [(g, (0x9E3779B1 * (i + 1)) & 0xFFFFFFFF or 1)
            for i, g in enumerate(gs)]


def check_report(rep, flips, expected_cells, cell_offset=0):
    """Exact accounting of planted corruption."""
    flat = expected_cells.reshape(-1)
    triples = {(4 * cell_offset + g, int(flat[g]), int(flat[g]) ^ m)
               for g, m in flips}
    assert rep.bad_dwords == len(flips)
    assert rep.bad_bits == sum(bin(m).count("1") for _, m in flips)
    assert rep.first_bad_dword == 4 * cell_offset + min(g for g, _ in flips)
    assert rep.xor_or == functools.reduce(lambda a, b: a | b,
                                          (m for _, m in flips))
    assert not rep.clean
    assert len(set(rep.log)) == len(rep.log)
    if len(flips) <= ops.MEM_LOG_SLOTS:
        assert set(rep.log) == triples
    else:
        assert len(rep.log) == ops.MEM_LOG_SLOTS
        assert set(rep.log) <= triples


@pytest.mark.parametrize("nontemporal", [True, False])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_cells", SIZES)
def test_fill_matches_reference(n_cells, pattern, invert, nontemporal):
    buf = new_buf(n_cells)
    ops.mem_fill(buf, pattern, SEED, invert, nontemporal=nontemporal)
    assert np.array_equal(cells(buf), ref(pattern, SEED, invert, n_cells))


def test_fill_leaves_neighbours_alone():
    """A 257-cell fill inside a larger tensor writes exactly its cells."""
    big = new_buf(257 + 64)
    ops.mem_fill(big[128:128 + 257 * 4], ADDR, SEED)
    got = cells(big)
    assert np.array_equal(got[32:32 + 257], ref(ADDR, SEED, False, 257))
    assert (got[:32] == 0x5A5A5A5A).all() and (got[289:] == 0x5A5A5A5A).all()


def test_any_dtype_buffer():
    buf = torch.zeros(785 * 16, dtype=torch.uint8, device=DEV)
    ops.mem_fill(buf, WALK, 7)
    assert np.array_equal(cells(buf), ref(WALK, 7, False, 785))


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_cells", SIZES)
def test_clean_verify(n_cells, pattern, invert):
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, pattern, SEED, invert)
    ops.mem_verify(buf, report, pattern, SEED, invert)
    raw = report.cpu().tolist()
    assert raw[2] == -1 and raw[:2] == [0, 0] and not any(raw[3:])
    rep = ops.mem_report_read(report)
    assert rep.clean and rep.first_bad_dword is None
    assert (rep.bad_dwords, rep.bad_bits, rep.xor_or, rep.log) == (0, 0, 0, [])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_cells", SIZES)
def test_planted_corruption(n_cells, pattern):
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, pattern, SEED)
    flips = standard_flips(n_cells)
    plant(buf, flips)
    ops.mem_verify(buf, report, pattern, SEED)
    check_report(ops.mem_report_read(report), flips,
                 ref(pattern, SEED, False, n_cells))


@pytest.mark.parametrize("n_cells", [65, 785, 65536])
def test_planted_corruption_overflows_log(n_cells):
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, ADDR, SEED)
    flips = many_flips(n_cells)
    plant(buf, flips)
    ops.mem_verify(buf, report, ADDR, SEED)
    check_report(ops.mem_report_read(report), flips,
                 ref(ADDR, SEED, False, n_cells))


def test_fully_corrupt_buffer():
    """Every dword wrong: counts stay exact and the log stays bounded."""
    n_cells = 65536
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, ADDR, SEED)
    ops.mem_verify(buf, report, ADDR, SEED, invert=True)
    rep = ops.mem_report_read(report)
    assert rep.bad_dwords == 4 * n_cells
    assert rep.bad_bits == 32 * 4 * n_cells
    assert rep.first_bad_dword == 0 and rep.xor_or == 0xFFFFFFFF
    assert len(rep.log) == ops.MEM_LOG_SLOTS
    flat = ref(ADDR, SEED, True, n_cells).reshape(-1)
    for g, expected, actual in rep.log:
        assert expected == int(flat[g]) and actual == expected ^ 0xFFFFFFFF


VF_CASES = [((ADDR, SEED, False), (ADDR, SEED, True)),
            ((ADDR, SEED, True), (WALK, 5, False)),
            ((WALK, 5, False), (CHECKER, 9, True))]


@pytest.mark.parametrize("nontemporal", [True, False])
@pytest.mark.parametrize("old,new", VF_CASES)
@pytest.mark.parametrize("n_cells", SIZES)
def test_verify_fill(n_cells, old, new, nontemporal):
    # clean: nothing reported, buffer ends as `new`
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, *old)
    ops.mem_verify_fill(buf, report, old, new, nontemporal=nontemporal)
    assert ops.mem_report_read(report).clean
    assert np.array_equal(cells(buf), ref(*new, n_cells))
    # corrupted beforehand: reported exactly, buffer still ends as `new`
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, *old)
    flips = standard_flips(n_cells)
    plant(buf, flips)
    ops.mem_verify_fill(buf, report, old, new, nontemporal=nontemporal)
    check_report(ops.mem_report_read(report), flips, ref(*old, n_cells))
    assert np.array_equal(cells(buf), ref(*new, n_cells))


def test_cell_offset_slice():
    buf = new_buf(4096)
    ops.mem_fill(buf, ADDR, SEED)
    tail = buf[4 * 1000:]
    report = ops.mem_report_new(DEV)
    ops.mem_verify(tail, report, ADDR, SEED, cell_offset=1000)
    assert ops.mem_report_read(report).clean
    ops.mem_verify(tail, report, ADDR, SEED, cell_offset=0)
    rep = ops.mem_report_read(report)
    assert not rep.clean
    # ADDR cells are pairwise distinct, so every cell of the slice differs
    assert rep.bad_dwords >= 3096


@pytest.mark.parametrize("pattern", PATTERNS)
def test_64bit_cell_offset(pattern):
    off, n_cells = 2**33 + 5, 785
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, pattern, SEED, cell_offset=off)
    expected = ref(pattern, SEED, False, n_cells, off)
    assert np.array_equal(cells(buf), expected)
    ops.mem_verify(buf, report, pattern, SEED, cell_offset=off)
    assert ops.mem_report_read(report).clean
    # global dword indices past 2^32 come back intact
    flips = standard_flips(n_cells)
    plant(buf, flips)
    ops.mem_verify(buf, report, pattern, SEED, cell_offset=off)
    check_report(ops.mem_report_read(report), flips, expected,
                 cell_offset=off)


def test_report_accumulates():
    n_cells = 257
    buf = new_buf(n_cells)
    report = ops.mem_report_new(DEV)
    ops.mem_fill(buf, CHECKER, 1)
    flips = standard_flips(n_cells)
    plant(buf, flips)
    ops.mem_verify(buf, report, CHECKER, 1)
    ops.mem_verify(buf, report, CHECKER, 1)
    rep = ops.mem_report_read(report)
    assert rep.bad_dwords == 2 * len(flips)
    assert rep.bad_bits == 2 * sum(bin(m).count("1") for _, m in flips)
    assert rep.first_bad_dword == 0
    assert len(rep.log) == 2 * len(flips)


def test_gpu_argument_validation():
    buf = new_buf(64)
    good = ops.mem_report_new(DEV)
    with pytest.raises(RuntimeError, match="int64"):
        ops.mem_verify(buf, good.to(torch.int32), ADDR, 0)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        ops.mem_verify(buf, good[:-1], ADDR, 0)
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.mem_verify(buf, good.cpu(), ADDR, 0)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.mem_verify(buf, good, 3, 0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.mem_fill(buf[1:5], ADDR, 0)
    # nothing above may have launched: the buffer is untouched
    assert (buf == 0x5A5A5A5A).all()


def test_memtest_march():
    buf = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rep, moved = memtest(buf, passes=2)
    assert rep.clean and rep.first_bad_dword is None and rep.log == []
    assert moved == 2 * 8 * (1 << 20)
    # the march ends on CHECKER with the last pass's seed (seed + 1)
    assert np.array_equal(cells(buf), ref(CHECKER, 1, False, (1 << 20) // 16))


def _run_memtest(*extra):
    proc = subprocess.run([str(MI_STREAM), "--memtest", "--mib", "64",
                           *extra],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1])


def test_mi_stream_memtest_clean():
    proc, j = _run_memtest()
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "memtest selftest: detector caught 3/3 injected flips" \
        in proc.stdout
    assert j["payload"] == "mi-memtest"
    assert j["bytes"] == 64 << 20 and j["passes"] == 1
    assert j["mem_clean"] is True and j["bad_dwords"] == 0
    assert j["bad_bits"] == 0 and j["first_bad_byte"] == -1
    assert j["xor_or"] == "0x00000000"


def test_mi_stream_memtest_inject():
    proc, j = _run_memtest("--memtest-inject", "3")
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert j["mem_clean"] is False
    assert j["bad_bits"] == 3 and j["bad_dwords"] == 3
    assert j["first_bad_byte"] == 0  # first flip is at cell 0
    assert j["xor_or"] == "0x00000007"  # bits 0, 1, 2
    # one log line per flip: byte offset / expected / actual / xor
    n_cells = (64 << 20) // 16
    offsets = {f"0x{16 * i * (n_cells // 3):016x}" for i in range(3)}
    logged = {ln.split()[0] for ln in proc.stdout.splitlines()
              if ln.startswith("0x")}
    assert logged == offsets
