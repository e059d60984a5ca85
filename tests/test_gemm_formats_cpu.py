"""Verified GEMM formats (fp16, int8, fp32, fp64), CPU side: the reference
product per format, the format table, report-index mapping for 64-bit
results, mi-stream's host-only validation and the Job manifest."""

import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops.gemmtest import locate, reference_operand, reference_product

REPO = Path(__file__).resolve().parent.parent
MI_STREAM = REPO / "native" / "bin" / "mi-stream"

FORMATS = ["fp16", "int8", "fp32", "fp64"]
RESULT = {"bf16": np.float32, "fp16": np.float32, "int8": np.int32,
          "fp32": np.float32, "fp64": np.float64}


@pytest.mark.parametrize("fmt", ["bf16"] + FORMATS)
def test_reference_product_per_format(fmt):
    a = reference_operand(0, 7, 33, 70).astype(np.int64)
    b = reference_operand(1, 7, 70, 21).astype(np.int64)
    p = reference_product(7, 33, 21, 70, fmt=fmt)
    assert p.dtype == RESULT[fmt]
    assert np.array_equal(p.astype(np.int64), a @ b)
    assert np.array_equal(p, (a @ b).astype(RESULT[fmt]))


def test_reference_product_defaults_and_errors():
    assert reference_product(7, 8, 8, 8).dtype == np.float32  # bf16
    with pytest.raises(ValueError):
        reference_product(7, 8, 8, 8, fmt="fp8")
    for fmt in FORMATS:
        with pytest.raises(ValueError):
            reference_product(0, 128, 128, 32768 + 128, fmt=fmt)


def test_gemm_formats_table():
    assert ops.GEMM_FORMATS == {
        "bf16": (torch.bfloat16, torch.float32, 64),
        "fp16": (torch.float16, torch.float32, 64),
        "int8": (torch.int8, torch.int32, 128),
        "fp32": (torch.float32, torch.float32, 32),
        "fp64": (torch.float64, torch.float64, 16)}
    for operand, _, k_step in ops.GEMM_FORMATS.values():
        # one K-step is 128 bytes of every operand row
        assert k_step * torch.empty(0, dtype=operand).element_size() == 128


def test_locate_two_dwords_per_element():
    where = np.array([[8, 0x111], [9, 0x222], [0x13, 0x333], [4, -1]],
                     dtype=np.int32)  # 2 x 2 tiles of a 256 x 256 C
    for half in (0, 1):
        assert locate(half, 256, where, elem_dwords=2) == (0, 0, 0, 8, 0x111)
        assert locate(2 * (127 * 256 + 128) + half, 256, where,
                      elem_dwords=2) == (127, 128, 1, 9, 0x222)
        assert locate(2 * (128 * 256 + 127) + half, 256, where,
                      elem_dwords=2) == (128, 127, 2, 3, 0x333)
        assert locate(2 * (256 * 256 - 1) + half, 256, where,
                      elem_dwords=2) == (255, 255, 3, 4, 0xFFFFFFFF)
    # the default stays one dword per element
    assert locate(127 * 256 + 128, 256, where) == (127, 128, 1, 9, 0x222)


def _mi_stream(*args):
    return subprocess.run([str(MI_STREAM), "--gemmtest", *args],
                          capture_output=True, text=True, timeout=60)


def test_unknown_format_exits_2():
    """Refused before any HIP call; the message names every format's step."""
    proc = _mi_stream("--gemm-format", "bogus")
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
    assert "bogus" in proc.stderr
    for word in ("bf16 (K-step 64)", "fp16 (64)", "int8 (128)", "fp32 (32)",
                 "fp64 (16)"):
        assert word in proc.stderr


@pytest.mark.parametrize("fmt,k,k_step", [("fp16", 48, 64), ("int8", 64, 128),
                                          ("int8", 192, 128), ("fp32", 16, 32),
                                          ("fp32", 48, 32)])
def test_k_not_a_whole_step_exits_2(fmt, k, k_step):
    """K is a multiple of 16, which fp64 would take, but not of the chosen
    format's step. Host only."""
    assert k % 16 == 0 and k % k_step != 0
    proc = _mi_stream("--gemm-format", fmt, "--gemm-mnk", "128", "128", str(k))
    assert proc.returncode == 2, (proc.stdout, proc.stderr)
    assert f"--gemm-format {fmt}" in proc.stderr
    assert f"K a multiple of {k_step} " in proc.stderr


def test_fp64_refuses_half_a_step_and_the_cap():
    for k in ("24", "32784"):
        proc = _mi_stream("--gemm-format", "fp64", "--gemm-mnk", "128", "128",
                          k)
        assert proc.returncode == 2, (k, proc.stdout, proc.stderr)
        assert "K a multiple of 16 and <= 32768" in proc.stderr


def test_format_flag_needs_a_value():
    proc = _mi_stream("--gemm-format")
    assert proc.returncode == 2


def test_early_argument_validation():
    """Binding checks fire before any launch, so they work without a GPU."""
    for fn in (ops.gemm_dense_nt, ops.gemm_dense_ref_int):
        for fmt in FORMATS:
            dtype, _, s = ops.GEMM_FORMATS[fmt]
            z = lambda *shape: torch.zeros(*shape, dtype=dtype)  # noqa: E731
            with pytest.raises(RuntimeError, match=f"K % {s} == 0"):
                fn(z(128, s + s // 2), z(128, s + s // 2))
            with pytest.raises(RuntimeError, match="shape contract"):
                fn(z(64, s), z(128, s))  # M = 64
            with pytest.raises(RuntimeError, match="disagree on K"):
                fn(z(128, s), z(128, 2 * s))
            with pytest.raises(RuntimeError, match="must be on GPU"):
                fn(z(128, s), z(128, s))  # CPU tensors
        with pytest.raises(RuntimeError, match="must both be"):
            fn(torch.zeros(128, 64, dtype=torch.bfloat16),
               torch.zeros(128, 64, dtype=torch.bfloat16))
        with pytest.raises(RuntimeError, match="must both be"):
            fn(torch.zeros(128, 64), torch.zeros(128, 64, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="K <= 32768"):
        ops.gemm_dense_ref_int(torch.zeros(128, 32768 + 128, dtype=torch.int8),
                               torch.zeros(128, 32768 + 128, dtype=torch.int8))
    # gemm_fill: one 16-byte cell is 8 fp16, 16 int8, 4 fp32 or 2 fp64
    for dtype, per_cell in ((torch.float16, 8), (torch.int8, 16),
                            (torch.float32, 4), (torch.float64, 2)):
        with pytest.raises(RuntimeError, match=f"multiple of {per_cell}"):
            ops.gemm_fill(torch.zeros(8, per_cell // 2, dtype=dtype), 0, 0, 8,
                          per_cell // 2)
        with pytest.raises(RuntimeError, match="must be on GPU"):
            ops.gemm_fill(torch.zeros(8, per_cell, dtype=dtype), 0, 0, 8,
                          per_cell)
    with pytest.raises(RuntimeError, match="must be bfloat16"):
        ops.gemm_fill(torch.zeros(8, 8, dtype=torch.int32), 0, 0, 8, 8)


def test_formats_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-gemmtest-formats.yaml")
        .read_text()) if d]
    assert len(docs) == 4
    seen = []
    for job in docs:
        assert job["kind"] == "Job"
        assert job["spec"]["backoffLimit"] == 0
        pod = job["spec"]["template"]["spec"]
        assert pod["runtimeClassName"] == "amd"
        assert pod["restartPolicy"] == "Never"
        c = pod["containers"][0]
        assert c["resources"]["limits"]["amd.com/gpu"] == "1"
        cmd = c["command"]
        assert cmd[:3] == ["mi-stream", "--gemmtest", "--gemm-format"]
        fmt = cmd[3]
        assert job["metadata"]["name"] == f"mi-gemmtest-{fmt}"
        assert cmd[4:] == ["--gemm-size", "8192", "--gemm-seconds", "300"]
        seen.append(fmt)
    assert seen == FORMATS
