"""Host-link test, CPU side: the threaded host fill and verify and the chase
table (hostlink_pattern.h) against the independent numpy references,
binding-level argument checks, the sysfs link reader through
`mi-hostlink --link-info` on fixture trees, the payload's usage errors and
the Job manifest. Nothing here touches a GPU."""

import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops import hostlink as hl
from k3samd.ops.memtest import ADDR, CHECKER, WALK, reference_pattern

REPO = Path(__file__).resolve().parent.parent
MI_HOSTLINK = REPO / "native" / "bin" / "mi-hostlink"

SEED = 0xDEADBEEF12345678
PATTERNS = [ADDR, WALK, CHECKER]
SIZES = [1, 4097]
OFFSETS = [0, 2**32 + 5]
BDF = "0000:c1:00.0"

needs_native = pytest.mark.skipif(not ops.native_available(),
                                  reason="native extension not built")


@functools.lru_cache(maxsize=None)
def ref(pattern, invert, n_cells, cell_offset):
    r = reference_pattern(pattern, SEED, invert, n_cells, cell_offset)
    r.setflags(write=False)
    return r


def host_buf(n_cells):
    # poison so that a cell the fill skipped cannot match by accident
    return torch.full((16 * n_cells,), 0x5A, dtype=torch.uint8)


def words(buf):
    return buf.numpy().view(np.uint32)


def _run(*args):
    return subprocess.run([str(MI_HOSTLINK), *map(str, args)],
                          capture_output=True, text=True, timeout=60)


# ---- host fill / verify ----

@needs_native
@pytest.mark.parametrize("cell_offset", OFFSETS)
@pytest.mark.parametrize("n_cells", SIZES)
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_host_fill_matches_reference(pattern, invert, n_cells, cell_offset):
    buf = host_buf(n_cells)
    ops.link_host_fill(buf, pattern, SEED, invert, cell_offset)
    assert np.array_equal(words(buf).reshape(-1, 4),
                          ref(pattern, invert, n_cells, cell_offset))
    report = ops.link_host_verify(buf, pattern, SEED, invert, cell_offset)
    assert report.clean and report.bad_bits == 0
    assert report.first_bad_dword is None and report.log == []


@needs_native
@pytest.mark.parametrize("threads", [0, 1, 2, 3, 16])
@pytest.mark.parametrize("cell_offset", OFFSETS)
def test_host_verify_reports_planted_flips(cell_offset, threads):
    """First cell, last cell and one in the middle; the same answer from any
    number of workers, and the fill itself does not depend on it either."""
    n_cells = 4097
    buf = host_buf(n_cells)
    ops.link_host_fill(buf, ADDR, SEED, False, cell_offset, threads=threads)
    want = ref(ADDR, False, n_cells, cell_offset).reshape(-1)
    assert np.array_equal(words(buf), want)
    flips = [(1, 0x00000001), (4 * (n_cells // 2) + 2, 0x00010100),
             (4 * n_cells - 1, 0x80000000)]
    for g, mask in flips:
        words(buf)[g] ^= np.uint32(mask)
    report = ops.link_host_verify(buf, ADDR, SEED, False, cell_offset,
                                  threads=threads)
    assert report.bad_dwords == 3
    assert report.bad_bits == 1 + 2 + 1
    assert report.first_bad_dword == 4 * cell_offset + 1
    assert report.xor_or == 0x80010101
    assert report.log == [(4 * cell_offset + g, int(want[g]),
                           int(want[g]) ^ mask) for g, mask in flips]


@needs_native
def test_host_verify_log_is_the_sixteen_lowest():
    """More bad dwords than log slots: every count is exact and the log is
    the 16 lowest, whatever the split into worker ranges."""
    n_cells = 4097
    buf = host_buf(n_cells)
    ops.link_host_fill(buf, CHECKER, SEED)
    bad = list(range(5, 4 * n_cells, 401))  # 41 dwords
    for g in bad:
        words(buf)[g] ^= np.uint32(0xFFFFFFFF)
    for threads in (1, 5, 16):
        report = ops.link_host_verify(buf, CHECKER, SEED, threads=threads)
        assert report.bad_dwords == len(bad)
        assert report.bad_bits == 32 * len(bad)
        assert [rec[0] for rec in report.log] == bad[:16]


@needs_native
def test_host_verify_wrong_spec_fails_everywhere():
    buf = host_buf(64)
    ops.link_host_fill(buf, ADDR, SEED)
    assert ops.link_host_verify(buf, ADDR, SEED + 1).bad_dwords >= 64
    assert ops.link_host_verify(buf, ADDR, SEED, True).bad_dwords == 256


# ---- chase ----

@pytest.mark.parametrize("seed", [0, SEED])
@pytest.mark.parametrize("n", [2, 1024, 65536])
def test_reference_chase_cycle_visits_every_slot_once(n, seed):
    nxt = hl.reference_chase_table(n, seed)[:, 0]
    assert np.array_equal(np.sort(nxt), np.arange(n))  # a permutation
    seen = np.zeros(n, dtype=bool)
    i = 0
    for _ in range(n):
        i = int(nxt[i])
        assert not seen[i]
        seen[i] = True
    assert seen.all() and i == 0  # one cycle of length n, back at the start


def test_reference_chase_hand_values():
    """n = 2 alternates 1, 0, 1, ...; n = 8 with increment 5 by hand:
    0 -> 5 -> (0xB1 * 5 + 5) & 7 = 2 -> (0xB1 * 2 + 5) & 7 = 7."""
    assert hl.reference_chase(2, 0, 1) == (1, 1)
    assert hl.reference_chase(2, 0, 2) == (0, 1)
    assert hl.reference_chase(2, 0, 3) == (1, 0)
    assert hl.reference_chase(8, 5, 3) == (7, 5 ^ 2 ^ 7)
    assert hl.reference_chase(8, 4, 3) == (7, 5 ^ 2 ^ 7)  # increment is odd


@needs_native
@pytest.mark.parametrize("n", [2, 1024, 65536])
def test_chase_fill_and_expected_match_reference(n):
    table = torch.full((64 * n,), 0x5A, dtype=torch.uint8)
    ops.link_chase_fill(table, n, SEED)
    assert np.array_equal(words(table).reshape(n, 16),
                          hl.reference_chase_table(n, SEED))
    for hops in (1, n, 3 * n + 5):
        assert ops.link_chase_expected(n, SEED, hops) == \
            hl.reference_chase(n, SEED, hops)


def test_chase_dump_matches_reference():
    """The header as the payload compiles it; needs neither the extension
    nor a GPU (the dump returns before any HIP call)."""
    proc = _run("--pattern-dump", "chase", 1024, SEED, 3077)
    assert proc.returncode == 0, proc.stderr
    lines = proc.stdout.split("\n")
    assert tuple(map(int, lines[0].split())) == \
        hl.reference_chase(1024, SEED, 3077)
    assert [int(v) for v in lines[1:1025]] == \
        hl.reference_chase_table(1024, SEED)[:, 0].tolist()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_fill_dump_matches_reference(pattern):
    proc = _run("--pattern-dump", "fill", pattern, SEED, 1, 2**32 + 5, 70)
    assert proc.returncode == 0, proc.stderr
    got = np.array([[int(w, 16) for w in line.split()]
                    for line in proc.stdout.splitlines()], dtype=np.uint32)
    assert np.array_equal(got, reference_pattern(pattern, SEED, True, 70,
                                                 2**32 + 5))


# ---- argument validation ----

@needs_native
def test_early_argument_validation():
    """Every rule fires before any launch, so it can be checked without a
    GPU: an unpinned tensor stands in for the host buffer wherever another
    rule comes first."""
    buf = torch.zeros(64, dtype=torch.uint8)
    cpu_report = torch.zeros(ops.MEM_REPORT_LEN, dtype=torch.int64)
    cpu_out = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.link_pull_verify(buf, cpu_report, 3, 0)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.link_push_fill(buf, -1, 0)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.link_host_fill(buf, 3, 0)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.link_host_verify(buf, 3, 0)
    for wgs in (0, 4097):
        with pytest.raises(RuntimeError, match=r"wgs must be in 1 \.\. 4096"):
            ops.link_pull_verify(buf, cpu_report, ADDR, 0, wgs=wgs)
        with pytest.raises(RuntimeError, match=r"wgs must be in 1 \.\. 4096"):
            ops.link_push_fill(buf, ADDR, 0, wgs=wgs)
    for wgs in (1, 4097):
        with pytest.raises(RuntimeError,
                           match=r"duplex wgs must be in 2 \.\. 4096"):
            ops.link_duplex(buf[:32], cpu_report, (ADDR, 0, False), buf[32:],
                            (ADDR, 0, False), wgs=wgs)
    for bad in (torch.zeros(15, dtype=torch.uint8),
                torch.zeros(0, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="non-zero multiple of 16"):
            ops.link_push_fill(bad, ADDR, 0)
        with pytest.raises(RuntimeError, match="non-zero multiple of 16"):
            ops.link_pull_verify(bad, cpu_report, ADDR, 0)
        with pytest.raises(RuntimeError, match="non-zero multiple of 16"):
            ops.link_host_fill(bad, ADDR, 0)
        with pytest.raises(RuntimeError, match="non-zero multiple of 16"):
            ops.link_host_verify(bad, ADDR, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.link_push_fill(torch.zeros(8, 8)[:, ::2], ADDR, 0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.link_host_fill(torch.zeros(36, dtype=torch.uint8)[4:], ADDR, 0)
    with pytest.raises(RuntimeError, match="int64"):
        ops.link_pull_verify(buf, cpu_report.to(torch.int32), ADDR, 0)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        ops.link_pull_verify(buf, cpu_report[:55], ADDR, 0)
    with pytest.raises(RuntimeError, match="report must be on GPU"):
        ops.link_pull_verify(buf, cpu_report, ADDR, 0)
    with pytest.raises(RuntimeError, match="report must be on GPU"):
        ops.link_duplex(buf[:32], cpu_report, (ADDR, 0, False), buf[32:],
                        (ADDR, 0, False))
    # overlap: identical, partial, and nested regions
    for pull, push in ((buf, buf), (buf[:48], buf[32:]), (buf, buf[16:32])):
        with pytest.raises(RuntimeError, match="must not overlap"):
            ops.link_duplex(pull, cpu_report, (ADDR, 0, False), push,
                            (ADDR, 0, False))
    for n in (0, 1, 3, 1 << 27):
        with pytest.raises(RuntimeError, match="power of two in 2"):
            ops.link_chase(buf, n, 1, cpu_out)
        with pytest.raises(RuntimeError, match="power of two in 2"):
            ops.link_chase_fill(buf, n, 0)
        with pytest.raises(RuntimeError, match="power of two in 2"):
            ops.link_chase_expected(n, 0, 1)
    for hops in (0, -1, (1 << 22) + 1):
        with pytest.raises(RuntimeError, match="hops must be in 1"):
            ops.link_chase(buf, 2, hops, cpu_out)
        with pytest.raises(RuntimeError, match="hops must be in 1"):
            ops.link_chase_expected(2, 0, hops)
    with pytest.raises(RuntimeError, match=r"byte size must be 64 \* n"):
        ops.link_chase(buf, 2, 1, cpu_out)  # 64 bytes, n = 2 needs 128
    with pytest.raises(RuntimeError, match=r"byte size must be 64 \* n"):
        ops.link_chase_fill(buf, 2, 0)
    with pytest.raises(RuntimeError, match=r"out must be a contiguous int64"):
        ops.link_chase(torch.zeros(128, dtype=torch.uint8), 2, 1, cpu_out[:3])
    with pytest.raises(RuntimeError, match="out must be on GPU"):
        ops.link_chase(torch.zeros(128, dtype=torch.uint8), 2, 1, cpu_out)
    with pytest.raises(RuntimeError, match="threads must be 0"):
        ops.link_host_fill(buf, ADDR, 0, threads=17)
    with pytest.raises(RuntimeError, match="threads must be 0"):
        ops.link_host_verify(buf, ADDR, 0, threads=-1)
    with pytest.raises(ValueError, match="power of two"):
        hl.reference_chase(3, 0, 1)


@needs_native
def test_python_constants_match_the_extension():
    from k3samd import _C
    assert ops.LINK_DEFAULT_WGS == _C.LINK_DEFAULT_WGS
    assert ops.LINK_MAX_WGS == _C.LINK_MAX_WGS


@needs_native
def test_unpinned_buffer_refused_without_a_gpu():
    """push_fill takes no GPU tensor, so its pinned check is reachable
    here: pageable memory is refused by name."""
    buf = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must be pinned"):
        ops.link_push_fill(buf, ADDR, 0)
    assert not buf.any()


# ---- the sysfs link reader, through mi-hostlink --link-info ----

def _link_tree(root, cur_speed=None, cur_width=None, max_speed=None,
               max_width=None, **extra):
    d = root / "bus" / "pci" / "devices" / BDF
    d.mkdir(parents=True)
    files = {"current_link_speed": cur_speed, "current_link_width": cur_width,
             "max_link_speed": max_speed, "max_link_width": max_width, **extra}
    for name, value in files.items():
        if value is not None:
            (d / name).write_text(f"{value}\n")
    return root


def _link_info(root):
    proc = _run("--link-info", "--sysfs-root", root, "--bdf", BDF)
    assert proc.returncode == 0, proc.stderr
    return json.loads(proc.stdout)


def test_link_info_full_gen5_x16(tmp_path):
    j = _link_info(_link_tree(tmp_path, "32.0 GT/s PCIe", 16,
                              "32.0 GT/s PCIe", 16, numa_node=1,
                              pcie_replay_count=7))
    assert j["bdf"] == BDF and j["link_known"] is True
    assert (j["link_gen"], j["link_width"]) == (5, 16)
    assert (j["link_max_gen"], j["link_max_width"]) == (5, 16)
    assert j["link_degraded"] is False
    # 32 GT/s x 16 lanes / 8 bits x 128/130 = 63.015...
    assert j["link_raw_gbps"] == pytest.approx(32 * 16 / 8 * 128 / 130,
                                               abs=0.05)
    assert j["link_raw_gbps"] == pytest.approx(63.0, abs=0.05)
    assert j["numa_node"] == 1 and j["pcie_replay_count"] == 7


def test_link_info_half_width_is_degraded(tmp_path):
    j = _link_info(_link_tree(tmp_path, "32.0 GT/s PCIe", 8,
                              "32.0 GT/s PCIe", 16))
    assert (j["link_gen"], j["link_width"]) == (5, 8)
    assert j["link_degraded"] is True
    assert j["link_raw_gbps"] == pytest.approx(31.5, abs=0.05)


def test_link_info_lower_speed_is_degraded(tmp_path):
    j = _link_info(_link_tree(tmp_path, "16.0 GT/s PCIe", 16,
                              "32.0 GT/s PCIe", 16))
    assert (j["link_gen"], j["link_max_gen"]) == (4, 5)
    assert j["link_degraded"] is True
    assert j["link_raw_gbps"] == pytest.approx(31.5, abs=0.05)


def test_link_info_old_kernel_format_and_gen2_encoding(tmp_path):
    """Kernels before 5.x print "5 GT/s"; Gen1-2 use 8b/10b encoding."""
    j = _link_info(_link_tree(tmp_path, "5 GT/s", 4, "5 GT/s", 4))
    assert (j["link_gen"], j["link_width"]) == (2, 4)
    assert j["link_degraded"] is False
    assert j["link_raw_gbps"] == pytest.approx(5 * 4 / 8 * 0.8, abs=0.05)


def test_link_info_absent_files_read_unknown(tmp_path):
    """Missing files, a missing device and "Unknown" all read as unknown:
    neither an error nor a healthy link, and never degraded by default."""
    for root in (_link_tree(tmp_path / "a"),
                 tmp_path / "nothing-here",
                 _link_tree(tmp_path / "b", "Unknown", 0, "Unknown", 0)):
        j = _link_info(root)
        assert j["link_known"] is False
        assert j["link_gen"] == -1 and j["link_width"] == -1
        assert j["link_raw_gbps"] == -1.0
        assert j["link_degraded"] is False
        assert j["numa_node"] == -1 and j["pcie_replay_count"] == -1


def test_link_info_writes_nothing(tmp_path):
    root = _link_tree(tmp_path, "32.0 GT/s PCIe", 16, "32.0 GT/s PCIe", 16)
    before = sorted((p, p.read_bytes() if p.is_file() else None)
                    for p in root.rglob("*"))
    _link_info(root)
    assert before == sorted((p, p.read_bytes() if p.is_file() else None)
                            for p in root.rglob("*"))


# ---- CLI ----

@pytest.mark.parametrize("args", [
    ["--bogus"], ["--mib"], ["--mib", 0], ["--mib", 65537], ["--passes", 0],
    ["--wgs", 0], ["--wgs", 4097], ["--chase-hops", 0],
    ["--chase-hops", (1 << 22) + 1], ["--inject", 0], ["--inject", 17],
    ["--min-gbps", 0], ["--min-gbps", -3], ["--device", -1],
    ["--link-info"], ["--bdf", BDF], ["--sysfs-root", "/sys"],
    ["--pattern-dump"], ["--pattern-dump", "fill", 3, 0, 0, 0, 1],
    ["--pattern-dump", "chase", 3, 0, 1], ["--pattern-dump", "other", 1, 2, 3],
])
def test_usage_errors_exit_2_before_hip(args):
    """Exit 2 comes before any HIP call: on a machine without a GPU a HIP
    call would have exited 1 instead."""
    proc = _run(*args)
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
    assert "hip" not in proc.stderr.lower().replace("mi-hostlink", "")


def test_help_lists_every_flag():
    proc = _run("--help")
    assert proc.returncode == 0
    for flag in ("--device", "--mib", "--passes", "--wgs", "--chase-hops",
                 "--inject", "--require-full-link", "--min-gbps",
                 "--pattern-dump", "--link-info", "--sysfs-root", "--bdf"):
        assert flag in proc.stdout, flag


# ---- packaging ----

def test_hostlink_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-hostlink.yaml").read_text()) if d]
    assert len(docs) == 1
    job = docs[0]
    assert job["kind"] == "Job"
    assert job["metadata"]["name"] == "mi-hostlink"
    assert job["spec"]["backoffLimit"] == 0
    pod = job["spec"]["template"]["spec"]
    assert pod["runtimeClassName"] == "amd"
    assert pod["restartPolicy"] == "Never"
    c = pod["containers"][0]
    assert c["resources"]["limits"]["amd.com/gpu"] == "1"
    assert c["command"] == ["mi-hostlink", "--mib", "1024", "--passes", "2",
                            "--require-full-link"]


def test_hostlink_is_shipped():
    assert "/src/native/bin/mi-hostlink" in (
        REPO / "deploy" / "docker" / "Dockerfile").read_text()
    assert "mi-hostlink" in (
        REPO / "deploy" / "scripts" / "install-node.sh").read_text()
