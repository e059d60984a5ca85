"""Verified GEMM for the fp16, int8, fp32 and fp64 matrix pipes on the GPU:
the fill, the MFMA kernel and the integer gold kernel of every format,
each bitwise against the numpy product; layout, bound, wide-range and
general-data checks independent of the generator; the drivers and
mi-stream --gemmtest --gemm-format.

S is the format's K-step (128 bytes of a row). Shapes are the smallest at
which the kernels can still go wrong: one tile with one, two and an odd
number of K-steps, two tiles along either axis, a non-square
non-power-of-two grid, and 256 blocks."""

import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops.gemmtest import (gemmtest, locate, reference_operand,
                                 reference_product)

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_STREAM = REPO / "native" / "bin" / "mi-stream"

DEV = "cuda:0"
SEED = 0xDEADBEEF12345678
FORMATS = ["fp16", "int8", "fp32", "fp64"]
INT32_MIN = -2 ** 31


def step(fmt):
    return ops.GEMM_FORMATS[fmt][2]


def shapes(fmt):
    s = step(fmt)
    return [(128, 128, s), (128, 128, 2 * s), (128, 128, 3 * s),
            (256, 128, s), (128, 256, s), (384, 640, 5 * s), (2048, 2048, s)]


# (format, shape index) pairs, so that every case names its format
CASES = [pytest.param(fmt, i, id=f"{fmt}-{i}")
         for fmt in FORMATS for i in range(7)]


@functools.lru_cache(maxsize=None)
def ref_product(fmt, m, n, k):
    """Reference computed once per format and shape; returned read-only."""
    r = reference_product(SEED, m, n, k, fmt=fmt)
    r.setflags(write=False)
    return r


def operands(fmt, m, n, k, seed=SEED):
    dtype = ops.GEMM_FORMATS[fmt][0]
    a = torch.empty((m, k), dtype=dtype, device=DEV)
    bt = torch.empty((n, k), dtype=dtype, device=DEV)
    ops.gemm_fill(a, 0, seed, m, k)
    ops.gemm_fill(bt, 1, seed, n, k)
    return a, bt


def poisoned(fmt, m, n):
    """NaN, or INT32_MIN for int8 (-1 is a legitimate product), so that an
    element the kernel skipped cannot match by accident."""
    dtype = ops.GEMM_FORMATS[fmt][1]
    value = INT32_MIN if dtype == torch.int32 else float("nan")
    return torch.full((m, n), value, dtype=dtype, device=DEV)


def all_poison(t):
    if t.dtype == torch.int32:
        return bool((t == INT32_MIN).all())
    return bool(torch.isnan(t).all())


def bits(x):
    """Bit patterns of a tensor or array as unsigned integers."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)


def assert_bitwise(c, expected):
    assert c.cpu().numpy().dtype == expected.dtype
    got, want = bits(c), bits(expected)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} element(s) differ, first at "
                           f"{bad[0].tolist()}: got "
                           f"{c[tuple(bad[0])].item()}, want "
                           f"{expected[tuple(bad[0])]}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n,steps", [(128, 64, 1), (384, 128, 5)])
def test_fill_matches_reference(fmt, m, n, steps):
    k = steps * step(fmt)
    a, bt = operands(fmt, m, n, k)
    assert np.array_equal(a.cpu().numpy().astype(np.int32),
                          reference_operand(0, SEED, m, k))
    # Bt[n][k] holds logical B[k][n]
    assert np.array_equal(bt.cpu().numpy().astype(np.int32),
                          reference_operand(1, SEED, k, n).T)


@pytest.mark.parametrize("fmt,i", CASES)
def test_mfma_gemm_exact(fmt, i):
    m, n, k = shapes(fmt)[i]
    a, bt = operands(fmt, m, n, k)
    c = poisoned(fmt, m, n)
    where = None
    if i == 6:
        where = torch.full((256, 2), -1, dtype=torch.int32, device=DEV)
    out = ops.gemm_dense_nt(a, bt, out=c, where=where)
    assert out.data_ptr() == c.data_ptr()
    assert_bitwise(c, ref_product(fmt, m, n, k))
    if where is not None:
        w = where.cpu().numpy()
        # every tile wrote its record (a row still at -1/-1 was skipped)
        assert not ((w[:, 0] == -1) & (w[:, 1] == -1)).any()
        xcc = w[:, 0] & 0xF  # XCC id: low 4 bits of the XCC_ID register
        assert ((xcc >= 0) & (xcc <= 7)).all()


@pytest.mark.parametrize("fmt,i", CASES)
def test_ref_int_exact(fmt, i):
    m, n, k = shapes(fmt)[i]
    a, bt = operands(fmt, m, n, k)
    gold = poisoned(fmt, m, n)
    ops.gemm_dense_ref_int(a, bt, out=gold)
    assert_bitwise(gold, ref_product(fmt, m, n, k))


@pytest.mark.parametrize("fmt", FORMATS)
def test_allocating_form(fmt):
    m, n, k = 128, 256, step(fmt)
    a, bt = operands(fmt, m, n, k)
    for fn in (ops.gemm_dense_nt, ops.gemm_dense_ref_int):
        c = fn(a, bt)
        assert c.shape == (m, n) and c.dtype == ops.GEMM_FORMATS[fmt][1]
        assert_bitwise(c, ref_product(fmt, m, n, k))


@pytest.mark.parametrize("fmt", FORMATS)
def test_identity_layout(fmt):
    """Layout check independent of the generator: A = I with an asymmetric
    random Bt of values the format holds exactly must reproduce Bt
    transposed, exactly. K = 128 is a whole number of steps in every
    format. This pins the C/D map, that of the f64 form included."""
    operand, result, _ = ops.GEMM_FORMATS[fmt]
    g = torch.Generator().manual_seed(1)
    a = torch.eye(128, dtype=operand, device=DEV)
    if fmt == "int8":
        bt = torch.randint(-128, 128, (256, 128), generator=g,
                           dtype=torch.int8).to(DEV)
    else:
        bt = torch.randn(256, 128, generator=g,
                         dtype=torch.float64).to(operand).to(DEV)
    c = poisoned(fmt, 128, 256)
    ops.gemm_dense_nt(a, bt, out=c)
    assert torch.equal(c, bt.T.to(result))


@pytest.mark.parametrize("fn", [ops.gemm_dense_nt, ops.gemm_dense_ref_int],
                         ids=["mfma", "ref_int"])
@pytest.mark.parametrize("fmt", ["fp16", "fp32"])
def test_bound_case(fmt, fn):
    """K = 32768 with every operand -16: each sum reaches 2^23, the limit
    of the exactness argument. Then one element of A becomes 15 and only
    its row changes: 2^23 - (-16)(-16) + 15*(-16) = 8388112."""
    m, n, k = 128, 128, 32768
    dtype = ops.GEMM_FORMATS[fmt][0]
    a = torch.full((m, k), -16.0, dtype=dtype, device=DEV)
    bt = torch.full((n, k), -16.0, dtype=dtype, device=DEV)
    c = poisoned(fmt, m, n)
    fn(a, bt, out=c)
    assert (bits(c) == np.float32(2 ** 23).view(np.uint32)).all()
    a[5, 777] = 15.0
    c = poisoned(fmt, m, n)
    fn(a, bt, out=c)
    want = np.full((m, n), 2.0 ** 23, dtype=np.float32)
    want[5, :] = 8388112.0
    assert np.array_equal(c.cpu().numpy(), want)


@pytest.mark.parametrize("fn", [ops.gemm_dense_nt, ops.gemm_dense_ref_int],
                         ids=["mfma", "ref_int"])
def test_int8_full_range(fn):
    """Uniform operands over all of [-128, 127], bitwise against a numpy
    int64 product: |sum| <= 640 * 2^14 < 2^24, far inside int32."""
    m, n, k = 256, 384, 640
    rng = np.random.default_rng(3)
    a = rng.integers(-128, 128, (m, k), dtype=np.int8)
    bt = rng.integers(-128, 128, (n, k), dtype=np.int8)
    assert a.min() == -128 and a.max() == 127
    c = poisoned("int8", m, n)
    fn(torch.from_numpy(a).to(DEV), torch.from_numpy(bt).to(DEV), out=c)
    want = a.astype(np.int64) @ bt.astype(np.int64).T
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want)


def test_fp64_wide_integers():
    """Uniform integer operands in [-2^20, 2^20], bitwise against a numpy
    int64 product: |sum| <= 512 * 2^40 = 2^49 < 2^53, so every partial sum
    is exact in fp64 under any association, and the products exercise
    mantissa bits the generator's 5-bit operands never reach."""
    m, n, k = 256, 384, 512
    rng = np.random.default_rng(4)
    a = rng.integers(-2 ** 20, 2 ** 20 + 1, (m, k), dtype=np.int64)
    bt = rng.integers(-2 ** 20, 2 ** 20 + 1, (n, k), dtype=np.int64)
    c = poisoned("fp64", m, n)
    ops.gemm_dense_nt(torch.from_numpy(a.astype(np.float64)).to(DEV),
                      torch.from_numpy(bt.astype(np.float64)).to(DEV), out=c)
    got = c.cpu().numpy()
    want = a @ bt.T
    assert np.abs(want).max() < 2 ** 53
    assert np.array_equal(got, want.astype(np.float64))
    assert np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("fmt", ["fp16", "fp32"])
def test_general_data(fmt):
    """Random normal data against a float64 product. Bound: the standard
    gamma_K accumulation bound |C - C64| <= K*u*(|A|.|B|) with u = 2^-23
    (which allows a truncating adder), 1 % slack for the higher-order
    terms: derived, not tuned — the bound of the bf16 test."""
    m, n, k = 256, 384, 512
    dtype = ops.GEMM_FORMATS[fmt][0]
    g = torch.Generator().manual_seed(2)
    a = torch.randn(m, k, generator=g).to(dtype)
    bt = torch.randn(n, k, generator=g).to(dtype)
    c = poisoned(fmt, m, n)
    ops.gemm_dense_nt(a.to(DEV), bt.to(DEV), out=c)
    a64, b64 = a.double().numpy(), bt.double().numpy().T
    c64 = a64 @ b64
    bound = 1.01 * k * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64))
    err = np.abs(c.cpu().numpy().astype(np.float64) - c64)
    print(f"max err {err.max():.3e}, max err/bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


# ---- driver ----

def plant(buf, flips):
    """XOR mask into 32-bit dword d of the buffer for every (d, mask)."""
    idx = torch.tensor([d for d, _ in flips], dtype=torch.int64, device=DEV)
    masks = np.array([m for _, m in flips], dtype=np.uint32).view(np.int32)
    flat = buf.view(torch.int32).view(-1)
    flat[idx] = flat[idx] ^ torch.from_numpy(masks).to(DEV)


@pytest.mark.parametrize("fmt", FORMATS)
def test_gemmtest_driver_clean(fmt):
    k = 2 * step(fmt)
    rep, flops, where = gemmtest(256, 256, k, iters=3, seed=SEED, fmt=fmt)
    assert rep.clean and rep.first_bad_dword is None and rep.log == []
    assert flops == 3 * 2.0 * 256 * 256 * k
    assert where.shape == (4, 2) and where.dtype == np.int32
    assert not ((where[:, 0] == -1) & (where[:, 1] == -1)).any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_gemmtest_driver_locates_planted_bit(fmt):
    """For fp64 the bit goes into the HIGH dword of the element (half 1):
    report dword 2 * element + 1."""
    k = 2 * step(fmt)
    row, col = 200, 77  # tile (1, 0) of the 2 x 2 grid
    dwords = 2 if fmt == "fp64" else 1
    index = (row * 256 + col) * dwords + (dwords - 1)
    rep, _, where = gemmtest(
        256, 256, k, iters=2, seed=SEED, fmt=fmt,
        gold_hook=lambda gold: plant(gold, [(index, 0x00000100)]))
    assert rep.bad_dwords == 2 and rep.bad_bits == 2  # once per iteration
    assert rep.first_bad_dword == index and rep.xor_or == 0x100
    elem = int(bits(ref_product(fmt, 256, 256, k))[row, col])
    want = (elem >> 32) if fmt == "fp64" else elem
    # the log holds (index, gold bits, C bits): gold carries the flip
    assert set(rep.log) == {(index, want ^ 0x100, want)}
    r, c, tile, xcc, hw_id = locate(rep.first_bad_dword, 256, where,
                                    elem_dwords=dwords)
    assert (r, c, tile) == (row, col, 2)
    assert 0 <= xcc <= 7
    assert hw_id == int(where[2][1]) & 0xFFFFFFFF


@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_argument_validation_launches_nothing(fmt):
    s = step(fmt)
    operand, result, _ = ops.GEMM_FORMATS[fmt]
    a, bt = operands(fmt, 128, 128, 2 * s)
    c = poisoned(fmt, 128, 128)
    wrong = torch.float64 if result != torch.float64 else torch.float32
    other = torch.float32 if operand != torch.float32 else torch.float64
    name = {torch.float32: "float32", torch.int32: "int32",
            torch.float64: "float64"}[result]
    for fn in (ops.gemm_dense_nt, ops.gemm_dense_ref_int):
        with pytest.raises(RuntimeError, match=f"out must be {name}"):
            fn(a, bt, out=c.to(wrong))
        with pytest.raises(RuntimeError, match="shape contract.*K % "
                           f"{s} == 0"):
            # one and a half steps
            fn(a[:, :s + s // 2].contiguous(), bt[:, :s + s // 2].contiguous(),
               out=c)
        with pytest.raises(RuntimeError, match="must both be"):
            fn(a, bt.to(other), out=c)
        with pytest.raises(RuntimeError, match="must be on GPU"):
            fn(a, bt.cpu(), out=c)
        with pytest.raises(RuntimeError, match="same GPU"):
            fn(a, bt, out=c.cpu())
        with pytest.raises(RuntimeError, match=r"out must be \[M,N\]"):
            fn(a, bt, out=poisoned(fmt, 128, 256))
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            fn(a, bt, out=poisoned(fmt, 128, 129).view(-1)[1:1 + 128 * 128]
               .view(128, 128))
    with pytest.raises(RuntimeError, match="where must be int32"):
        ops.gemm_dense_nt(a, bt, out=c, where=torch.zeros(
            (1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"int32\[tiles,2\]"):
        ops.gemm_dense_nt(a, bt, out=c, where=torch.zeros(
            (2, 2), dtype=torch.int32, device=DEV))
    # nothing above may have launched: the output is still all poison
    assert all_poison(c)


# ---- mi-stream --gemmtest --gemm-format ----

def _run_gemmtest(fmt, *extra):
    proc = subprocess.run([str(MI_STREAM), "--gemmtest", "--gemm-format", fmt,
                           "--gemm-size", "512", "--gemm-iters", "4", *extra],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_mi_stream_gemmtest_clean(fmt):
    proc, j = _run_gemmtest(fmt)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert (f"gemmtest selftest: 256x256x{2 * step(fmt)} {fmt} MFMA product "
            "and integer gold match the host product exactly") in proc.stdout
    assert "gemmtest selftest: detector caught 3/3 injected flips" \
        in proc.stdout
    assert f"gemmtest: {fmt} 512x512x512, gold by integer VALU" in proc.stdout
    assert "spot-check 64/64 vs host" in proc.stdout
    assert j["payload"] == "mi-gemmtest" and j["format"] == fmt
    assert (j["m"], j["n"], j["k"], j["iters"]) == (512, 512, 512, 4)
    assert j["compute_clean"] is True
    assert j["bad_elems"] == 0 and j["bad_bits"] == 0
    assert (j["first_bad_row"], j["first_bad_col"], j["first_bad_xcc"]) == \
        (-1, -1, -1)
    # the member order log parsers see: "format" directly after "payload"
    pairs = json.loads(proc.stdout.strip().splitlines()[-1],
                       object_pairs_hook=list)
    assert [key for key, _ in pairs] == [
        "payload", "format", "m", "n", "k", "iters", "bad_elems", "bad_bits",
        "first_bad_row", "first_bad_col", "first_bad_xcc", "avg_tflops",
        "gold_ms", "max_temp_c", "max_power_w", "compute_clean"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_mi_stream_gemmtest_inject(fmt):
    """Flip i sits at element i * (M*N // 3), bit i: one log line each. In
    an fp64 element the flip helper writes the LOW dword: half 0."""
    proc, j = _run_gemmtest(fmt, "--gemm-inject", "3")
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert j["format"] == fmt and j["compute_clean"] is False
    assert j["bad_elems"] == 3 and j["bad_bits"] == 3
    assert (j["first_bad_row"], j["first_bad_col"]) == (0, 0)
    assert 0 <= j["first_bad_xcc"] <= 7
    elems = [i * (512 * 512 // 3) for i in range(3)]
    want = {(e // 512, e % 512, 1 << i) for i, e in enumerate(elems)}
    pat = re.compile(r"^C\[(\d+)\]\[(\d+)\] expected 0x[0-9a-f]{8} actual "
                     r"0x[0-9a-f]{8} xor 0x([0-9a-f]{8}) xcc (\d) "
                     r"hw_id 0x[0-9a-f]{8}"
                     + (" half 0$" if fmt == "fp64" else "$"))
    logged = {(int(mt[1]), int(mt[2]), int(mt[3], 16))
              for mt in map(pat.match, proc.stdout.splitlines()) if mt}
    assert logged == want


def test_mi_stream_gemmtest_explicit_bf16():
    """The flag with bf16 runs today's bf16 test; only the JSON gains the
    format member."""
    proc, j = _run_gemmtest("bf16")
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "gemmtest: 512x512x512, gold by integer VALU" in proc.stdout
    assert j["format"] == "bf16" and j["compute_clean"] is True
