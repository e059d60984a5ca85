"""GPU tests for the standalone in-pod payload binaries (mi-stream,
mi-allreduce) — the executables the smoke manifests run where the
reference ran `nvidia-smi` (/root/reference/nvidia-smi.yaml:13)."""

import json
import subprocess
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
BIN = REPO / "native" / "bin"

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="no GPU")


@requires_gpu
def test_mi_stream_runs():
    proc = subprocess.run([str(BIN / "mi-stream"), "--mib", "512",
                           "--iters", "5"],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    # built-in numerics oracle must have run and passed (exit 3 otherwise)
    assert "numerics: triad exact" in proc.stdout
    assert "MX-fp8 identity exact" in proc.stdout
    last = proc.stdout.strip().splitlines()[-1]
    j = json.loads(last)
    assert j["payload"] == "mi-stream"
    assert j["arch"].startswith("gfx950")
    # >L3 buffers on MI355X must stream well past 4 TB/s
    assert j["triad_gbps"] > 4000, j
    assert j["mfma_bf16_tflops"] > 500, j


@requires_gpu
def test_mi_stream_all_gpus():
    proc = subprocess.run([str(BIN / "mi-stream"), "--all-gpus",
                           "--mib", "256", "--iters", "5"],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    last = proc.stdout.strip().splitlines()[-1]
    j = json.loads(last)
    assert j["mode"] == "all-gpus"
    assert j["n_gpus"] >= 1
    assert j["aggregate_triad_gbps"] > 4000 * j["n_gpus"]


@requires_gpu
def test_mi_stream_burn_short():
    proc = subprocess.run([str(BIN / "mi-stream"), "--burn", "4",
                           "--mib", "256"],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    j = json.loads(proc.stdout.strip().splitlines()[-1])
    assert j["payload"] == "mi-burn"
    assert j["avg_triad_gbps"] > 2000  # concurrent with MFMA load
    assert j["avg_mfma_tflops"] > 50


def _mi_stream_small(*flags):
    """One mi-stream mode at 64 MiB x 2 iterations: the buffers sit in
    cache there, so these tests assert structure, never a rate floor."""
    proc = subprocess.run([str(BIN / "mi-stream"), "--mib", "64",
                           "--iters", "2", *flags],
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    return proc.stdout.strip().splitlines()


@requires_gpu
def test_mi_stream_lds_compare():
    lines = _mi_stream_small("--lds-compare")
    assert any(ln.startswith("numerics: triad exact") for ln in lines)
    j = json.loads(lines[-1])
    assert j["payload"] == "mi-stream-lds"
    assert j["direct_gbps"] > 0 and j["lds_staged_gbps"] > 0, j


@requires_gpu
def test_mi_stream_tune():
    lines = _mi_stream_small("--tune")
    assert "tune: grid-stride nt triad, 64 MiB buffers" in lines
    assert ["tpb", "unroll", "blocks", "GB/s"] in [ln.split() for ln in lines]
    assert not any(ln.startswith("{") for ln in lines)  # no JSON line
    rows = [ln.split() for ln in lines if " U1 " in ln]
    # 3 block sizes x 4 occupancies: tpb, unroll, blocks, U1 r, U2 r, U4 r
    assert [(int(r[0]), int(r[2])) for r in rows] == \
        [(tpb, 256 * waves * 64 // tpb)
         for tpb in (256, 512, 1024) for waves in (4, 8, 16, 32)]
    for r in rows:
        assert r[3:9:2] == ["U1", "U2", "U4"], r
        assert all(float(rate) > 0 for rate in r[4:9:2]), r


@requires_gpu
def test_mi_stream_no_mfma_no_check():
    lines = _mi_stream_small("--no-mfma", "--no-check")
    assert not any("numerics:" in ln for ln in lines)
    assert not any("MFMA" in ln for ln in lines)
    j = json.loads(lines[-1])
    assert j["payload"] == "mi-stream"
    assert j["mfma_bf16_tflops"] == 0.0


@requires_gpu
def test_mi_allreduce_single_gpu():
    proc = subprocess.run([str(BIN / "mi-allreduce"), "--ngpus", "1",
                           "--min-mib", "4", "--max-mib", "16",
                           "--iters", "5"],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    last = proc.stdout.strip().splitlines()[-1]
    j = json.loads(last)
    assert j["payload"] == "mi-allreduce"
    assert j["n_gpus"] == 1


@requires_gpu
def test_mi355x_smi_real_sysfs():
    """mi355x-smi against the real /sys of the GPU box."""
    proc = subprocess.run([str(BIN / "mi355x-smi"), "--json"],
                          capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    j = json.loads(proc.stdout)
    assert j["gpu_count"] >= 1
    g = j["gpus"][0]
    assert g["arch"] == "gfx950"
    assert g["vram_bytes"] > 200 * (1 << 30)
    assert g["render_minor"] >= 128
    # health/RAS fields present (values depend on the box's driver build;
    # -1 = not exposed is acceptable, absence is not)
    for key in ("ras_supported", "ras_uncorrectable", "ras_correctable",
                "ras_deferred", "fatal_ras_events", "retired_vram_pages",
                "pcie_replay_count", "reset_count"):
        assert key in g, key
    if g["ras_supported"] == "true":
        # the MI355X pool exposes ACA RAS banks: counters must be real
        # numbers (not the -1 'absent' sentinel) once RAS is present
        assert g["ras_uncorrectable"] >= 0
        assert g["ras_correctable"] >= 0
        assert g["ras_deferred"] >= 0


@pytest.mark.gpu
def test_mi355x_smi_topo_real():
    """--topo connectivity matrix renders on the real box (single-GPU
    lease: one row, no peer columns marked XGMI unless peers are
    visible KFD nodes)."""
    proc = subprocess.run([str(BIN / "mi355x-smi"), "--topo"],
                          capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    assert "GPU0" in proc.stdout
    assert "Legend" in proc.stdout
