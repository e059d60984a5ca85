"""Verified MX GEMM, CPU side: the host operand and scale generator
(mi-mxgemm's dumps, compiled from mx_pattern.h) against the independent
numpy reference, the encodings, the exactness bounds, binding-level argument
checks, the payload's usage errors and the Job manifest."""

import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops.mxgemmtest import (E4M3_VALUES, FP4_VALUES, pack_codes,
                                   reference_elements, reference_product,
                                   reference_scales, scaled_operands)

REPO = Path(__file__).resolve().parent.parent
MI_MXGEMM = REPO / "native" / "bin" / "mi-mxgemm"

FP8, FP4 = ops.MX_FMT_FP8, ops.MX_FMT_FP4
FMT_NAME = {FP8: "fp8", FP4: "fp4"}
ROWS, COLS = 5, 19  # window dumped at each origin
SEEDS = [0, 0xDEADBEEF12345678]
ORIGINS = [(0, 0), (127, 63), (8191, 4095)]


def _run(*args):
    return subprocess.run([str(MI_MXGEMM), *map(str, args)],
                          capture_output=True, text=True, timeout=60)


def _dump(*args):
    proc = _run(*args)
    assert proc.returncode == 0, proc.stderr
    return np.array([[int(w) for w in line.split()]
                     for line in proc.stdout.splitlines()], dtype=np.int64)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("fmt", [FP8, FP4])
def test_operand_dump_matches_reference(fmt, which, origin, seed):
    """Runs without a GPU: the dump returns before any HIP call."""
    got = _dump("--operand-dump", FMT_NAME[fmt], which, seed, *origin, ROWS,
                COLS)
    _, codes = reference_elements(fmt, which, seed, ROWS, COLS, *origin)
    assert got.shape == (ROWS, COLS)
    assert np.array_equal(got, codes)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("which", [0, 1])
def test_scale_dump_matches_reference(which, origin, seed):
    got = _dump("--scale-dump", which, seed, *origin, ROWS, COLS)
    ref = reference_scales(which, seed, ROWS, COLS, *origin)
    assert got.shape == (ROWS, COLS)
    assert np.array_equal(got, ref)


def test_dumps_reject_bad_arguments():
    assert _run("--operand-dump", "fp6", 0, 0, 0, 0, 1, 1).returncode == 2
    assert _run("--operand-dump", "fp8", 2, 0, 0, 0, 1, 1).returncode == 2
    assert _run("--scale-dump", 2, 0, 0, 0, 1, 1).returncode == 2


def test_e4m3_anchor_encodings():
    """0 -> 0x00, 1 -> 0x38 (exponent field 7 = bias), 15 -> 0x57
    (1.111b x 2^3), -16 -> 0xD8 (sign, exponent field 11). Checked on the
    decode table, and on the host encoder through a generated window that
    holds every value -16..15."""
    assert E4M3_VALUES[0x00] == 0 and E4M3_VALUES[0x38] == 1
    assert E4M3_VALUES[0x57] == 15 and E4M3_VALUES[0xD8] == -16
    assert np.isnan(E4M3_VALUES[0x7F]) and np.isnan(E4M3_VALUES[0xFF])
    assert E4M3_VALUES[0x7E] == 448  # largest finite e4m3fn
    values, codes = reference_elements(FP8, 0, 3, 16, 64)
    want = {0: 0x00, 1: 0x38, 15: 0x57, -16: 0xD8}
    dumped = _dump("--operand-dump", "fp8", 0, 3, 0, 0, 16, 64)
    for v, byte in want.items():
        assert (values == v).any()
        assert set(codes[values == v]) == {byte}
        assert set(dumped[values == v]) == {byte}
    # every byte the generator emits decodes to an integer in range
    assert set(np.unique(values)) == set(range(-16, 16))
    assert np.array_equal(E4M3_VALUES[dumped], values)


def test_fp4_code_table():
    assert FP4_VALUES[:8].tolist() == [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    assert FP4_VALUES[8:].tolist() == [-0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    assert np.isfinite(FP4_VALUES).all()
    # e2m1: 1 sign, 2 exponent (bias 1), 1 mantissa bit
    for code in range(16):
        e, m = (code >> 1) & 3, code & 1
        mag = m * 0.5 if e == 0 else (1 + m * 0.5) * 2.0 ** (e - 1)
        assert abs(FP4_VALUES[code]) == mag
        assert np.signbit(FP4_VALUES[code]) == bool(code & 8)


def test_generator_range_and_asymmetry():
    for which in (0, 1):
        v8, _ = reference_elements(FP8, which, 0x1234, 512, 512)
        assert v8.min() == -16 and v8.max() == 15
        assert not np.array_equal(v8, v8.T)  # a transposed operand must show
        v4, c4 = reference_elements(FP4, which, 0x1234, 512, 512)
        assert set(np.unique(c4)) == set(range(16))
        assert not np.array_equal(c4, c4.T)
        s = reference_scales(which, 0x1234, 512, 256)
        assert set(np.unique(s)) == {127, 128}
    for fmt in (FP8, FP4):
        a = reference_elements(fmt, 0, 0x1234, 64, 64)[1]
        b = reference_elements(fmt, 1, 0x1234, 64, 64)[1]
        assert not np.array_equal(a, b.T) and not np.array_equal(a, b)
    assert not np.array_equal(reference_scales(0, 0x1234, 64, 64),
                              reference_scales(1, 0x1234, 64, 64))


def test_scales_are_not_the_element_hash():
    """The scale of (r, block) must not follow the element at (r, col =
    block): with the same hash, scale 128 would coincide with the top
    element bit."""
    _, codes = reference_elements(FP4, 0, 9, 256, 256)
    s = reference_scales(0, 9, 256, 256)
    agree = ((codes >> 3) == (s - 127)).mean()
    assert 0.4 < agree < 0.6


def test_exactness_bounds():
    """fp8: |scaled| <= 32, |a*b| <= 1024, 1024*K = 2^23 at K = 8192.
    fp4: scaled <= 24 halves, product <= 576 quarters, 576*8192 < 2^23.
    Below 2^24 fp32 holds every integer."""
    k = ops.MX_EXACT_MAX_K
    assert k == 8192
    assert 16 * 2 == 32 and 32 * 32 * k == 2 ** 23
    assert 6 * 2 * 2 == 24 and 24 * 24 == 576 and 576 * k < 2 ** 23
    assert np.float32(2 ** 23) + np.float32(1) == np.float32(2 ** 23 + 1)
    for fmt in (FP8, FP4):
        a, b = scaled_operands(fmt, 5, 64, 64, 256)
        limit = 32 if fmt == FP8 else 12
        assert np.abs(a).max() <= limit and np.abs(b).max() <= limit
        with pytest.raises(ValueError):
            reference_product(fmt, 0, 128, 128, k + 256)


@pytest.mark.parametrize("fmt", [FP8, FP4])
def test_reference_product_is_integer_matmul(fmt):
    """Against an explicit int64 product of the scaled operands, in units
    of 1 (fp8) or, for fp4, halves per operand = quarters per product."""
    m, n, k = 33, 21, 96
    per = 1 if fmt == FP8 else 2
    v_a, _ = reference_elements(fmt, 0, 7, m, k)
    v_b, _ = reference_elements(fmt, 1, 7, k, n)
    sa = reference_scales(0, 7, m, k // 32).astype(np.int64) - 127
    sb = reference_scales(1, 7, n, k // 32).astype(np.int64) - 127
    a = (v_a * per).astype(np.int64) << np.repeat(sa, 32, axis=1)
    b = (v_b * per).astype(np.int64) << np.repeat(sb, 32, axis=1).T
    assert np.array_equal(a, v_a * per * 2.0 ** np.repeat(sa, 32, axis=1))
    p = reference_product(fmt, 7, m, n, k)
    assert p.dtype == np.float32
    assert np.array_equal(p.astype(np.float64) * per * per, a @ b)


def test_pack_codes():
    codes = np.array([[1, 2, 0xF, 0]], dtype=np.uint8)
    assert pack_codes(FP8, codes).tolist() == [[1, 2, 0xF, 0]]
    assert pack_codes(FP4, codes).tolist() == [[0x21, 0x0F]]  # low = even k


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


def test_early_argument_validation():
    """Binding checks fire before any launch, so they work without a GPU."""
    if not ops.native_available():
        pytest.skip("native extension not built")
    good = (_u8(128, 128), _u8(128, 4), _u8(128, 128), _u8(128, 4))
    for fn in (ops.mx_gemm_nt, ops.mx_gemm_ref_int):
        with pytest.raises(RuntimeError, match="fmt must be"):
            fn(*good, 2)
        with pytest.raises(RuntimeError, match="2-D uint8"):
            fn(torch.zeros(128, 128), *good[1:], FP8)
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(_u8(64, 128), _u8(64, 4), *good[2:], FP8)  # M = 64
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(*good[:2], _u8(192, 128), _u8(192, 4), FP8)  # N = 192
        with pytest.raises(RuntimeError, match="shape contract"):
            fn(_u8(128, 192), _u8(128, 6), _u8(128, 192), _u8(128, 6), FP8)
        with pytest.raises(RuntimeError, match="shape contract"):
            # 64 bytes of fp4 = K 128: fp4 needs K % 256
            fn(_u8(128, 64), _u8(128, 4), _u8(128, 64), _u8(128, 4), FP4)
        with pytest.raises(RuntimeError, match="disagree on K"):
            fn(*good[:2], _u8(128, 256), _u8(128, 8), FP8)
        with pytest.raises(RuntimeError, match=r"SA \[M, K/32\]"):
            fn(good[0], _u8(128, 8), *good[2:], FP8)
        with pytest.raises(RuntimeError, match=r"SA \[M, K/32\]"):
            fn(*good[:3], _u8(64, 4), FP8)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(_u8(128, 256)[:, ::2], *good[1:], FP8)
        with pytest.raises(RuntimeError, match="must be on GPU"):
            fn(*good, FP8)  # CPU tensors
        with pytest.raises(RuntimeError, match="must be on GPU"):
            # the same bytes as fp4: K = 256, so 8 scale blocks per row
            fn(good[0], _u8(128, 8), good[2], _u8(128, 8), FP4)
    with pytest.raises(RuntimeError, match="K <= 8192"):
        ops.mx_gemm_ref_int(_u8(128, 8320), _u8(128, 260), _u8(128, 8320),
                            _u8(128, 260), FP8)
    with pytest.raises(RuntimeError, match="K <= 8192"):
        ops.mx_gemm_ref_int(_u8(128, 4224), _u8(128, 264), _u8(128, 4224),
                            _u8(128, 264), FP4)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.mx_gemm_nt(_u8(128 * 128 + 16)[1:-15].view(128, 128), *good[1:],
                       FP8)
    with pytest.raises(RuntimeError, match="which must be"):
        ops.mx_fill(_u8(8, 32), _u8(8, 1), 2, 0, 8, 32, FP8)
    with pytest.raises(RuntimeError, match="fmt must be"):
        ops.mx_fill(_u8(8, 32), _u8(8, 1), 0, 0, 8, 32, 1)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.mx_fill(_u8(8, 16), _u8(8, 1), 0, 0, 8, 16, FP8)
    with pytest.raises(RuntimeError, match="rows \\* k elements"):
        ops.mx_fill(_u8(8, 32), _u8(8, 1), 0, 0, 8, 32, FP4)  # fp4: 16 B/row
    with pytest.raises(RuntimeError, match="k / 32 bytes"):
        ops.mx_fill(_u8(8, 32), _u8(8, 2), 0, 0, 8, 32, FP8)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.mx_fill(_u8(8, 32), _u8(8, 1), 0, 0, 8, 32, FP8)
    tile = (_u8(16, 128), _u8(16, 4), _u8(16, 128), _u8(16, 4))
    with pytest.raises(RuntimeError, match="fmt must be"):
        ops.mx_gemm16_scaled(*tile, 3)
    with pytest.raises(RuntimeError, match=r"\[16,KB\]"):
        ops.mx_gemm16_scaled(*tile, FP4)  # fp4 tiles are [16,64]
    with pytest.raises(RuntimeError, match=r"\[16,4\]"):
        ops.mx_gemm16_scaled(tile[0], _u8(16, 1), *tile[2:], FP8)
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.mx_gemm16_scaled(*tile, FP8)


def test_driver_rejects_bad_format_before_touching_a_device():
    from k3samd.ops.mxgemmtest import mxgemmtest
    with pytest.raises(ValueError, match="fmt must be"):
        mxgemmtest(128, 128, 128, 2, device="cuda:99")


def test_usage_errors_exit_2():
    """Bad arguments are refused before any HIP call."""
    for extra in (["--size", "100"], ["--mnk", "128", "128", "192"],
                  ["--format", "fp4", "--mnk", "128", "128", "128"],
                  ["--size", "8320"],  # K over the exactness bound
                  ["--format", "fp4", "--mnk", "128", "128", "8448"],
                  ["--format", "fp6"], ["--inject", "17"], ["--inject", "0"],
                  ["--inject", "-1"], ["--iters", "2", "--seconds", "2"],
                  ["--bogus"], ["--size"]):
        proc = _run(*extra)
        assert proc.returncode == 2, (extra, proc.stdout, proc.stderr)


def test_help_prints_usage():
    proc = _run("--help")
    assert proc.returncode == 0
    for flag in ("--device", "--format fp8|fp4", "--size", "--mnk", "--iters",
                 "--seconds", "--inject", "--operand-dump", "--scale-dump"):
        assert flag in proc.stdout


def test_mxgemmtest_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-mxgemmtest.yaml").read_text())
        if d]
    assert [d["kind"] for d in docs] == ["Job", "Job"]
    for job, fmt in zip(docs, ("fp8", "fp4")):
        assert job["metadata"]["name"] == f"mi-mxgemmtest-{fmt}"
        assert job["spec"]["backoffLimit"] == 0
        pod = job["spec"]["template"]["spec"]
        assert pod["runtimeClassName"] == "amd"
        assert pod["restartPolicy"] == "Never"
        c = pod["containers"][0]
        assert c["resources"]["limits"]["amd.com/gpu"] == "1"
        assert c["command"] == ["mi-mxgemm", "--format", fmt, "--size", "8192",
                                "--seconds", "300"]


def test_payload_is_shipped():
    """The binary the manifest runs is in the image and the node install."""
    assert "/src/native/bin/mi-mxgemm" in (
        REPO / "deploy" / "docker" / "Dockerfile").read_text()
    assert "mi-mxgemm" in (
        REPO / "deploy" / "scripts" / "install-node.sh").read_text()
