"""HBM memory test, CPU side: the host pattern (mi-stream's dump, compiled
from memtest_pattern.h) against the independent numpy reference, pattern
injectivity, binding-level argument checks and the Job manifest."""

import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops.memtest import ADDR, CHECKER, WALK, reference_pattern

REPO = Path(__file__).resolve().parent.parent
MI_STREAM = REPO / "native" / "bin" / "mi-stream"

N_DUMP = 70  # > one wave of cells; crosses the 2^32 boundary at 2^32-1


def _dump(pattern, seed, invert, cell_offset, n_cells):
    proc = subprocess.run(
        [str(MI_STREAM), "--memtest-pattern-dump", str(pattern), str(seed),
         str(int(invert)), str(cell_offset), str(n_cells)],
        capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    rows = [[int(w, 16) for w in line.split()]
            for line in proc.stdout.splitlines()]
    return np.array(rows, dtype=np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF12345678])
@pytest.mark.parametrize("cell_offset",
                         [0, 1, 2**32 - 1, 2**32, 2**33 + 5])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", [ADDR, WALK, CHECKER])
def test_pattern_dump_matches_reference(pattern, invert, cell_offset, seed):
    """Runs without a GPU: the dump returns before any HIP call."""
    got = _dump(pattern, seed, invert, cell_offset, N_DUMP)
    ref = reference_pattern(pattern, seed, invert, N_DUMP, cell_offset)
    assert got.shape == (N_DUMP, 4)
    assert np.array_equal(got, ref)


def test_reference_spot_values():
    """Hand-evaluated anchors for the spec, independent of both
    implementations: lowbias32(0) = 0, the walking one, the checkerboard."""
    assert reference_pattern(ADDR, 0, False, 1).tolist() == \
        [[0, 0xFFFFFFFF, 0, 0]]
    # WALK: dword g holds 1 << ((g + seed) & 31); cell 8 starts at g = 32
    assert reference_pattern(WALK, 3, False, 1, 8).tolist() == \
        [[1 << 3, 1 << 4, 1 << 5, 1 << 6]]
    assert reference_pattern(CHECKER, 0, False, 2).tolist() == \
        [[0xAAAAAAAA, 0x55555555, 0xAAAAAAAA, 0x55555555],
         [0x55555555, 0xAAAAAAAA, 0x55555555, 0xAAAAAAAA]]
    assert reference_pattern(CHECKER, 0, True, 1).tolist() == \
        [[0x55555555, 0xAAAAAAAA, 0x55555555, 0xAAAAAAAA]]


@pytest.mark.parametrize("cell_offset", [0, 2**32 - 2**15])
def test_addr_pattern_injective(cell_offset):
    """ADDR cells are pairwise distinct over 2^16 consecutive cells (the
    second case straddles the lo32/hi32 boundary of the cell index)."""
    cells = reference_pattern(ADDR, 0x1234, False, 1 << 16, cell_offset)
    assert len(np.unique(cells, axis=0)) == 1 << 16


def test_early_argument_validation():
    """Binding checks fire before any launch, so they work without a GPU."""
    if not ops.native_available():
        pytest.skip("native extension not built")
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.mem_fill(torch.zeros(16, dtype=torch.uint8), ADDR, 0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.mem_fill(torch.zeros(15, dtype=torch.uint8), ADDR, 0)
    with pytest.raises(RuntimeError, match="unknown memtest pattern"):
        ops.mem_fill(torch.zeros(16, dtype=torch.uint8), 3, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.mem_fill(torch.zeros(8, 8)[:, ::2], ADDR, 0)
    report = torch.zeros(ops.MEM_REPORT_LEN, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.mem_verify(torch.zeros(4), report, ADDR, 0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.mem_verify_fill(torch.zeros(15, dtype=torch.uint8), report,
                            (ADDR, 0, False), (ADDR, 0, True))


def test_memtest_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-memtest.yaml").read_text()) if d]
    assert len(docs) == 1
    job = docs[0]
    assert job["kind"] == "Job"
    assert job["spec"]["backoffLimit"] == 0
    pod = job["spec"]["template"]["spec"]
    assert pod["runtimeClassName"] == "amd"
    assert pod["restartPolicy"] == "Never"
    c = pod["containers"][0]
    assert c["resources"]["limits"]["amd.com/gpu"] == "1"
    assert c["command"] == ["mi-stream", "--memtest", "--vram-percent", "90",
                            "--passes", "2"]
