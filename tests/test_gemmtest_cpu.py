"""Verified GEMM, CPU side: the host operand generator (mi-stream's dump,
compiled from gemm_pattern.h) against the independent numpy reference, the
exactness bound, binding-level argument checks and the Job manifest."""

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

ROWS, COLS = 5, 19  # window dumped at each origin


def _dump(which, seed, row0, col0, rows, cols):
    proc = subprocess.run(
        [str(MI_STREAM), "--gemm-operand-dump", str(which), str(seed),
         str(row0), str(col0), str(rows), str(cols)],
        capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    return np.array([[int(w) for w in line.split()]
                     for line in proc.stdout.splitlines()], dtype=np.int32)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF12345678])
@pytest.mark.parametrize("origin", [(0, 0), (127, 63), (32767, 4095)])
@pytest.mark.parametrize("which", [0, 1])
def test_operand_dump_matches_reference(which, origin, seed):
    """Runs without a GPU: the dump returns before any HIP call."""
    got = _dump(which, seed, *origin, ROWS, COLS)
    ref = reference_operand(which, seed, ROWS, COLS, *origin)
    assert got.shape == (ROWS, COLS)
    assert np.array_equal(got, ref)


def test_operand_dump_rejects_bad_which():
    proc = subprocess.run([str(MI_STREAM), "--gemm-operand-dump", "2", "0",
                           "0", "0", "1", "1"],
                          capture_output=True, text=True, timeout=60)
    assert proc.returncode == 2


def test_operand_anchor():
    """Hand-evaluated: row = col = seed = 0, which = 0 gives x = 0,
    lowbias32(0) = 0, so the value is (0 >> 27) - 16 = -16. For which = 1
    x = 0xA5A5A5A5, so A and B differ at the origin."""
    assert reference_operand(0, 0, 1, 1).tolist() == [[-16]]
    assert _dump(0, 0, 0, 0, 1, 1).tolist() == [[-16]]
    assert reference_operand(1, 0, 1, 1).tolist() != [[-16]]


def test_operand_range_and_asymmetry():
    for which in (0, 1):
        v = reference_operand(which, 0x1234, 512, 512)
        assert v.min() == -16 and v.max() == 15
        assert not np.array_equal(v, v.T)  # a transposed operand must show
    assert not np.array_equal(reference_operand(0, 0x1234, 64, 64),
                              reference_operand(1, 0x1234, 64, 64))


def test_exactness_bound():
    """|a*b| <= 256, so |sum| <= 256*K; at the largest accepted K that is
    exactly 2^23, below fp32's 2^24 integer limit."""
    assert ops.GEMM_EXACT_MAX_K == 32768
    assert 16 * 16 * ops.GEMM_EXACT_MAX_K == 2 ** 23
    assert np.float32(2 ** 23) + np.float32(1) == np.float32(2 ** 23 + 1)
    with pytest.raises(ValueError):
        reference_product(0, 128, 128, 32768 + 64)


def test_reference_product_is_integer_matmul():
    a = reference_operand(0, 7, 33, 70).astype(np.int64)
    b = reference_operand(1, 7, 70, 21).astype(np.int64)
    p = reference_product(7, 33, 21, 70)
    assert p.dtype == np.float32
    assert np.array_equal(p.astype(np.int64), a @ b)


def test_locate():
    where = np.array([[8, 0x111], [9, 0x222], [0x13, 0x333], [4, -1]],
                     dtype=np.int32)  # 2 x 2 tiles of a 256 x 256 C
    assert locate(0, 256, where) == (0, 0, 0, 8, 0x111)
    assert locate(127 * 256 + 128, 256, where) == (127, 128, 1, 9, 0x222)
    # XCC id is the low 4 bits of the register
    assert locate(128 * 256 + 127, 256, where) == (128, 127, 2, 3, 0x333)
    assert locate(256 * 256 - 1, 256, where) == (255, 255, 3, 4, 0xFFFFFFFF)


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def test_early_argument_validation():
    """Binding checks fire before any launch, so they work without a GPU."""
    if not ops.native_available():
        pytest.skip("native extension not built")
    for fn in (ops.gemm_bf16_nt, ops.gemm_ref_int):
        with pytest.raises(RuntimeError, match="must be bfloat16"):
            fn(torch.zeros(128, 64), _bf(128, 64))
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(_bf(64, 64), _bf(128, 64))  # M = 64
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(_bf(128, 64), _bf(192, 64))  # N = 192
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(_bf(128, 96), _bf(128, 96))  # K = 96
        with pytest.raises(RuntimeError, match="disagree on K"):
            fn(_bf(128, 64), _bf(128, 128))
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(_bf(128, 128)[:, ::2], _bf(128, 64))
        with pytest.raises(RuntimeError, match="must be on GPU"):
            fn(_bf(128, 64), _bf(128, 64))  # CPU tensors
    with pytest.raises(RuntimeError, match="K <= 32768"):
        ops.gemm_ref_int(_bf(128, 32832), _bf(128, 32832))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.gemm_bf16_nt(_bf(128 * 64 + 8)[1:-7].view(128, 64), _bf(128, 64))
    with pytest.raises(RuntimeError, match="which must be"):
        ops.gemm_fill(_bf(8, 8), 2, 0, 8, 8)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.gemm_fill(_bf(8, 4), 0, 0, 8, 4)
    with pytest.raises(RuntimeError, match="rows \\* cols"):
        ops.gemm_fill(_bf(8, 8), 0, 0, 8, 16)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.gemm_fill(_bf(8, 8), 0, 0, 8, 8)
    report = torch.zeros(ops.MEM_REPORT_LEN, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="same byte size"):
        ops.buf_compare(torch.zeros(8), torch.zeros(4), report)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.buf_compare(torch.zeros(3), torch.zeros(3), report)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.buf_compare(torch.zeros(4), torch.zeros(4), report)


def test_usage_errors_exit_2():
    """Bad --gemmtest arguments are refused before any HIP call."""
    for extra in (["--gemm-size", "100"], ["--gemm-mnk", "128", "128", "96"],
                  ["--gemm-mnk", "128", "128", "32832"],
                  ["--gemm-inject", "17"],
                  ["--gemm-iters", "2", "--gemm-seconds", "2"]):
        proc = subprocess.run([str(MI_STREAM), "--gemmtest", *extra],
                              capture_output=True, text=True, timeout=60)
        assert proc.returncode == 2, (extra, proc.stdout, proc.stderr)


def test_help_mentions_gemmtest():
    proc = subprocess.run([str(MI_STREAM), "--help"], capture_output=True,
                          text=True, timeout=60)
    assert proc.returncode == 0
    for flag in ("--gemmtest", "--gemm-size", "--gemm-mnk", "--gemm-iters",
                 "--gemm-seconds", "--gemm-inject", "--gemm-operand-dump"):
        assert flag in proc.stdout


def test_gemmtest_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-gemmtest.yaml").read_text()) if d]
    assert len(docs) == 1
    job = docs[0]
    assert job["kind"] == "Job"
    assert job["spec"]["backoffLimit"] == 0
    pod = job["spec"]["template"]["spec"]
    assert pod["runtimeClassName"] == "amd"
    assert pod["restartPolicy"] == "Never"
    c = pod["containers"][0]
    assert c["resources"]["limits"]["amd.com/gpu"] == "1"
    assert c["command"] == ["mi-stream", "--gemmtest", "--gemm-size", "8192",
                            "--gemm-seconds", "300"]
