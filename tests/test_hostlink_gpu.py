"""Host-link kernels on the GPU: pull, push, duplex and chase over pinned
host memory against the numpy references, exact accounting of planted
corruption, the pinned check, the phase driver and the mi-hostlink binary.

Sizes are the smallest at which the walk can still go wrong: one cell (a
single lane of a partial tile), 4097 cells (whole tiles for one workgroup
plus a one-cell tail; all tail for 3 and 64 workgroups) and 1 MiB = 65536
cells (whole tiles only for 1 and 64 workgroups, a ragged last tile for 3).
Every buffer sits inside a larger pinned allocation with guard cells on
both sides."""

import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops import hostlink as hl
from k3samd.ops.memtest import ADDR, CHECKER, WALK, reference_pattern

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_HOSTLINK = REPO / "native" / "bin" / "mi-hostlink"

SIZES = [1, 4097, 65536]
WGS = [1, 3, 64]
PATTERNS = [ADDR, WALK, CHECKER]
SEED = 0xDEADBEEF12345678
BIG_OFFSET = 2**32 + 5
DEV = "cuda:0"
GUARD = 4  # cells on either side of every region
POISON = 0xFF


@functools.lru_cache(maxsize=None)
def ref(pattern, seed, invert, n_cells, cell_offset=0):
    """Reference computed once per case and shared; returned read-only."""
    r = reference_pattern(pattern, seed, invert, n_cells, cell_offset)
    r.setflags(write=False)
    return r


def pinned_region(n_cells):
    """(whole, region): a poisoned pinned allocation and the view of its
    middle n_cells cells."""
    whole = torch.full((16 * (n_cells + 2 * GUARD),), POISON,
                       dtype=torch.uint8).pin_memory()
    return whole, whole[16 * GUARD:16 * (GUARD + n_cells)]


def words(buf):
    return buf.numpy().view(np.uint32)


def guards_intact(whole):
    w = whole.numpy()
    return bool((w[:16 * GUARD] == POISON).all()
                and (w[-16 * GUARD:] == POISON).all())


def standard_flips(n_cells):
    """Dword 0 (first cell), the last dword (last cell) and one in the
    middle."""
    flips = {0: 0x00000001, 4 * n_cells - 1: 0x80000000,
             4 * (n_cells // 2) + 2: 0x00010100}
    return sorted(flips.items())


def assert_flips_reported(report, flips, want, cell_offset=0):
    """`want` is the flat reference of the region."""
    base = 4 * cell_offset
    assert report.bad_dwords == len(flips)
    assert report.bad_bits == sum(bin(m).count("1") for _, m in flips)
    assert report.first_bad_dword == base + flips[0][0]
    xor_or = 0
    for _, m in flips:
        xor_or |= m
    assert report.xor_or == xor_or
    assert sorted(report.log) == [
        (base + g, int(want[g]), int(want[g]) ^ m) for g, m in flips]


# ---- pull ----

@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("n_cells", SIZES)
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pull_clean(pattern, invert, n_cells, wgs):
    _, buf = pinned_region(n_cells)
    words(buf)[:] = ref(pattern, SEED, invert, n_cells,
                        BIG_OFFSET).reshape(-1)
    report = ops.mem_report_new(DEV)
    ops.link_pull_verify(buf, report, pattern, SEED, invert, BIG_OFFSET,
                         wgs=wgs)
    got = ops.mem_report_read(report)
    assert got.clean and got.bad_bits == 0 and got.first_bad_dword is None


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("n_cells", SIZES)
@pytest.mark.parametrize("cell_offset", [0, BIG_OFFSET])
def test_pull_reports_planted_flips(cell_offset, n_cells, wgs):
    _, buf = pinned_region(n_cells)
    want = ref(ADDR, SEED, False, n_cells, cell_offset).reshape(-1)
    words(buf)[:] = want
    flips = standard_flips(n_cells)
    for g, mask in flips:
        words(buf)[g] ^= np.uint32(mask)
    report = ops.mem_report_new(DEV)
    ops.link_pull_verify(buf, report, ADDR, SEED, False, cell_offset, wgs=wgs)
    assert_flips_reported(ops.mem_report_read(report), flips, want,
                          cell_offset)


def test_pull_sees_a_host_write_between_two_launches():
    """The device must not serve the second pull from a cache: a flip the
    CPU plants after a clean pull is found by the next one."""
    n_cells = 4097
    _, buf = pinned_region(n_cells)
    want = ref(WALK, SEED, False, n_cells).reshape(-1)
    words(buf)[:] = want
    report = ops.mem_report_new(DEV)
    ops.link_pull_verify(buf, report, WALK, SEED, wgs=3)
    assert ops.mem_report_read(report).clean
    words(buf)[4 * 2000 + 1] ^= np.uint32(0x00000100)
    ops.link_pull_verify(buf, report, WALK, SEED, wgs=3)
    assert_flips_reported(ops.mem_report_read(report),
                          [(4 * 2000 + 1, 0x00000100)], want)


def test_pull_wrong_seed_fails_everywhere():
    n_cells = 4097
    _, buf = pinned_region(n_cells)
    words(buf)[:] = ref(ADDR, SEED, False, n_cells).reshape(-1)
    report = ops.mem_report_new(DEV)
    ops.link_pull_verify(buf, report, ADDR, SEED, True, wgs=3)
    got = ops.mem_report_read(report)
    assert got.bad_dwords == 4 * n_cells and got.bad_bits == 128 * n_cells
    assert got.first_bad_dword == 0 and got.xor_or == 0xFFFFFFFF
    assert len(got.log) == 16


# ---- push ----

@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("n_cells", SIZES)
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_push_exact_and_guards_untouched(pattern, invert, n_cells, wgs):
    whole, buf = pinned_region(n_cells)
    ops.link_push_fill(buf, pattern, SEED, invert, BIG_OFFSET, wgs=wgs)
    torch.cuda.synchronize()
    assert np.array_equal(words(buf).reshape(-1, 4),
                          ref(pattern, SEED, invert, n_cells, BIG_OFFSET))
    assert guards_intact(whole)


def test_push_then_host_verify_and_pull_agree():
    n_cells = 4097
    _, buf = pinned_region(n_cells)
    ops.link_push_fill(buf, CHECKER, SEED, wgs=3)
    torch.cuda.synchronize()
    assert ops.link_host_verify(buf, CHECKER, SEED).clean
    report = ops.mem_report_new(DEV)
    ops.link_pull_verify(buf, report, CHECKER, SEED, wgs=64)
    assert ops.mem_report_read(report).clean


# ---- duplex ----

@pytest.mark.parametrize("wgs", [2, 3, 7, 128])
@pytest.mark.parametrize("n_cells", SIZES)
def test_duplex_both_results_at_once(n_cells, wgs):
    """One launch: the planted flip in the pull region is found and the
    push region is exact, guards of both regions untouched."""
    pull_whole, pull = pinned_region(n_cells)
    push_whole, push = pinned_region(n_cells)
    want = ref(ADDR, SEED, False, n_cells).reshape(-1)
    words(pull)[:] = want
    flip = [(4 * (n_cells // 2) + 3, 0x00400000)]
    words(pull)[flip[0][0]] ^= np.uint32(flip[0][1])
    report = ops.mem_report_new(DEV)
    ops.link_duplex(pull, report, (ADDR, SEED, False), push,
                    (WALK, SEED + 1, True, BIG_OFFSET), wgs=wgs)
    assert_flips_reported(ops.mem_report_read(report), flip, want)
    assert np.array_equal(words(push).reshape(-1, 4),
                          ref(WALK, SEED + 1, True, n_cells, BIG_OFFSET))
    assert guards_intact(push_whole) and guards_intact(pull_whole)
    # the pull side wrote nothing
    expect_pull = want.copy()
    expect_pull[flip[0][0]] ^= np.uint32(flip[0][1])
    assert np.array_equal(words(pull), expect_pull)


def test_duplex_unequal_regions_and_clean_pull():
    _, pull = pinned_region(65536)
    push_whole, push = pinned_region(4097)
    words(pull)[:] = ref(CHECKER, SEED, True, 65536).reshape(-1)
    report = ops.mem_report_new(DEV)
    ops.link_duplex(pull, report, (CHECKER, SEED, True), push,
                    (ADDR, SEED, False), wgs=5)
    assert ops.mem_report_read(report).clean
    assert np.array_equal(words(push).reshape(-1, 4),
                          ref(ADDR, SEED, False, 4097))
    assert guards_intact(push_whole)


def test_duplex_overlap_refused_and_nothing_launched():
    whole, buf = pinned_region(64)
    report = ops.mem_report_new(DEV)
    before = report.clone()
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.link_duplex(buf, report, (ADDR, SEED, False), buf[16 * 8:16 * 24],
                        (ADDR, SEED, False))
    torch.cuda.synchronize()
    assert torch.equal(report, before)
    assert (whole.numpy() == POISON).all()


# ---- chase ----

def run_chase(table, n, hops):
    out = torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.link_chase(table, n, hops, out)
    return [int(v) for v in out.cpu().tolist()]


@pytest.mark.parametrize("n", [2, 1024])
def test_chase_matches_reference(n):
    table = torch.full((64 * n,), POISON, dtype=torch.uint8).pin_memory()
    ops.link_chase_fill(table, n, SEED)
    for hops in (1, n, 3 * n + 5):
        final, xor, ticks, got_hops = run_chase(table, n, hops)
        assert (final, xor) == hl.reference_chase(n, SEED, hops)
        assert (final, xor) == ops.link_chase_expected(n, SEED, hops)
        assert ticks > 0 and got_hops == hops


def test_chase_corrupt_slot_changes_the_answer_and_stays_in_bounds():
    """Slot 0's next overwritten with 0xFFFFFFFF: the mask turns it into
    slot n - 1, so the walk differs from the expectation, stays inside the
    table and the kernel returns normally."""
    n = 1024
    whole = torch.full((64 * (n + 2),), POISON, dtype=torch.uint8).pin_memory()
    table = whole[64:64 * (n + 1)]
    ops.link_chase_fill(table, n, SEED)
    nxt = hl.reference_chase_table(n, SEED)[:, 0].tolist()
    assert nxt[0] != n - 1
    words(table)[0] = np.uint32(0xFFFFFFFF)
    hops = 3 * n + 5
    final, xor, ticks, _ = run_chase(table, n, hops)
    assert (final, xor) != hl.reference_chase(n, SEED, hops)
    # what the masked walk must give, by hand
    nxt[0] = n - 1
    i = x = 0
    for _ in range(hops):
        i = nxt[i]
        x ^= i
    assert (final, xor) == (i, x) and ticks > 0
    torch.cuda.synchronize()
    assert (whole.numpy()[:64] == POISON).all()
    assert (whole.numpy()[-64:] == POISON).all()


# ---- pinned check ----

def test_unpinned_buffer_refused_and_nothing_launched():
    buf = torch.full((16 * 64,), POISON, dtype=torch.uint8)  # pageable
    assert not buf.is_pinned()
    report = ops.mem_report_new(DEV)
    report[:] = 0x5A5A  # poisoned: any launch would change it or the buffer
    before = report.clone()
    out = torch.full((4,), 0x5A5A, dtype=torch.int64, device=DEV)
    _, pinned = pinned_region(64)
    with pytest.raises(RuntimeError, match="pinned"):
        ops.link_pull_verify(buf, report, ADDR, SEED)
    with pytest.raises(RuntimeError, match="pinned"):
        ops.link_push_fill(buf, ADDR, SEED)
    with pytest.raises(RuntimeError, match="pinned"):
        ops.link_duplex(buf, report, (ADDR, SEED, False), pinned,
                        (ADDR, SEED, False))
    with pytest.raises(RuntimeError, match="pinned"):
        ops.link_duplex(pinned, report, (ADDR, SEED, False), buf,
                        (ADDR, SEED, False))
    with pytest.raises(RuntimeError, match="pinned"):
        ops.link_chase(buf, 16, 5, out)
    torch.cuda.synchronize()
    assert torch.equal(report, before)
    assert (out.cpu() == 0x5A5A).all()
    assert (buf.numpy() == POISON).all() and (pinned.numpy() == POISON).all()
    # and the device still works
    ops.link_push_fill(pinned, ADDR, SEED, wgs=1)
    torch.cuda.synchronize()
    assert np.array_equal(words(pinned).reshape(-1, 4),
                          ref(ADDR, SEED, False, 64))


def test_gpu_tensor_refused_as_host_buffer():
    with pytest.raises(RuntimeError, match="must be a CPU tensor"):
        ops.link_push_fill(torch.zeros(64, dtype=torch.uint8, device=DEV),
                           ADDR, SEED)


# ---- driver ----

def test_hostlink_driver_clean():
    result = hl.hostlink(mib=4, passes=1, seed=SEED, device=DEV,
                         chase_n=1024, chase_hops=2000)
    assert result.clean and result.bad_dwords == 0
    assert result.first_bad_phase is None
    assert set(result.phases) == set(hl.PHASES)
    for name, phase in result.phases.items():
        assert phase.report.clean, name
        assert phase.gbps > 0 and phase.ms > 0, name
        assert phase.bytes_moved == (4 << 20) * 4 * (
            2 if "duplex" in name else 1), name
    assert result.chase.ok and result.chase.hops == 2000
    assert result.chase.ticks > 0 and result.chase.ns_per_hop > 0


def test_hostlink_driver_inject():
    result = hl.hostlink(mib=4, passes=1, seed=3, device=DEV, inject=3,
                         chase_n=1024, chase_hops=100)
    assert not result.clean
    assert result.bad_dwords == 3 and result.bad_bits == 3
    assert result.first_bad_phase == "pull"
    pull = result.pull.report
    n_dwords = (4 << 20) // 4
    assert pull.bad_dwords == 3 and pull.first_bad_dword == 0
    assert sorted(g for g, _, _ in pull.log) == [0, (n_dwords - 1) // 2,
                                                 n_dwords - 1]
    assert pull.xor_or == 0b111
    for name in hl.PHASES[1:]:
        assert result.phases[name].report.clean, name
    assert result.chase.ok


# ---- mi-hostlink ----

JSON_KEYS = {"payload", "link_clean", "bad_dwords", "bad_bits",
             "first_bad_byte", "first_bad_phase", "pull_gbs", "push_gbs",
             "duplex_gbs", "h2d_gbs", "d2h_gbs", "sdma_duplex_gbs",
             "chase_ns", "link_gen", "link_width", "link_raw_gbps",
             "link_degraded", "pcie_replay_delta", "numa_node"}


def _payload(*args):
    proc = subprocess.run([str(MI_HOSTLINK), *map(str, args)],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.splitlines()
    return proc, lines, json.loads(lines[-1])


def test_mi_hostlink_clean():
    proc, lines, j = _payload("--mib", 16, "--passes", 1, "--chase-hops",
                              10000)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    selftest = [ln for ln in lines if ln.startswith("hostlink selftest:")]
    assert len(selftest) == 4 and not any("FAIL" in ln for ln in selftest)
    assert any("pull detector caught 3/3" in ln for ln in selftest)
    assert any("host detector caught 3/3" in ln for ln in selftest)
    assert any("1024-slot chase matches" in ln for ln in selftest)
    assert JSON_KEYS <= set(j)
    assert j["payload"] == "mi-hostlink" and j["link_clean"] is True
    assert j["bad_dwords"] == 0 and j["bad_bits"] == 0
    assert j["first_bad_byte"] == -1 and j["first_bad_phase"] == ""
    for key in ("pull_gbs", "push_gbs", "duplex_gbs", "h2d_gbs", "d2h_gbs",
                "sdma_duplex_gbs", "chase_ns"):
        assert j[key] > 0, key
    # one table row per phase and pass
    for phase in ("pull", "push", "duplex", "h2d", "d2h", "sdma-duplex"):
        assert sum(ln.split()[:2] == [phase, "0"] for ln in lines) == 1, phase
    # the replay counter is a delta or -1 (file absent), never a default 0
    # without the file; the link is read or reported unknown
    assert j["pcie_replay_delta"] >= -1
    assert j["link_gen"] in (-1, 1, 2, 3, 4, 5, 6)
    assert lines[0].startswith("mi-hostlink:") and "bdf" in lines[0]


def test_mi_hostlink_inject():
    proc, lines, j = _payload("--mib", 16, "--passes", 1, "--chase-hops",
                              1000, "--inject", 3)
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert j["link_clean"] is False
    assert j["bad_dwords"] == 3 and j["bad_bits"] == 3
    assert j["first_bad_byte"] == 0 and j["first_bad_phase"] == "pull"
    logged = [ln.split() for ln in lines
              if ln.startswith("0x") and len(ln.split()) == 5]
    assert len(logged) == 3 and all(rec[4] == "pull" for rec in logged)
    want = ref(ADDR, 0, False, (16 << 20) // 16).reshape(-1)
    n_dwords = len(want)
    for rec, (g, mask) in zip(sorted(logged, key=lambda r: int(r[0], 16)),
                              [(0, 1), ((n_dwords - 1) // 2, 2),
                               (n_dwords - 1, 4)]):
        assert int(rec[0], 16) == 4 * g
        assert int(rec[1], 16) == int(want[g])
        assert int(rec[2], 16) == int(want[g]) ^ mask
        assert int(rec[3], 16) == mask
