"""Verified MX (fp8 e4m3 / fp4 e2m1 block-scaled) MFMA GEMM on the GPU.

First the single tile with per-lane scales, which pins the lane -> scale
byte map everything else stands on; then layout checks that do not use the
generator; then the GEMM kernel and the integer reference kernel, each
bitwise against the numpy product; the bound case; the `where` table; the
driver; argument validation; and the mi-mxgemm payload.

Shapes are the smallest at which the kernels can still go wrong: one tile
with one, two and an odd number of K-steps, two tiles along either axis, a
non-square non-power-of-two grid, and 256 blocks. K counts K-steps of the
format: 128 k for fp8, 256 k for fp4 (128 bytes of a stored row)."""

import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops.mxgemmtest import (E4M3_VALUES, FP4_VALUES, locate,
                                   mxgemmtest, pack_codes, reference_elements,
                                   reference_product, reference_scales)

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_MXGEMM = REPO / "native" / "bin" / "mi-mxgemm"

DEV = "cuda:0"
SEED = 0xDEADBEEF12345678
FP8, FP4 = ops.MX_FMT_FP8, ops.MX_FMT_FP4
FMTS = pytest.mark.parametrize("fmt", [FP8, FP4], ids=["fp8", "fp4"])
STEP_K = {FP8: 128, FP4: 256}
VALUES = {FP8: E4M3_VALUES, FP4: FP4_VALUES}
ONE = {FP8: 0x38, FP4: 0x2}  # the code of 1.0
SHAPES = [(128, 128, 1), (128, 128, 2), (128, 128, 3), (256, 128, 1),
          (128, 256, 1), (384, 640, 5), (2048, 2048, 1)]
FNS = pytest.mark.parametrize("fn", [ops.mx_gemm_nt, ops.mx_gemm_ref_int],
                              ids=["mfma", "ref_int"])


@functools.lru_cache(maxsize=None)
def ref_product(fmt, m, n, k):
    """Reference computed once per shape and shared; returned read-only."""
    r = reference_product(fmt, SEED, m, n, k)
    r.setflags(write=False)
    return r


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def operands(fmt, m, n, k, seed=SEED):
    kb = k // 2 if fmt == FP4 else k
    a = torch.empty((m, kb), dtype=torch.uint8, device=DEV)
    bt = torch.empty((n, kb), dtype=torch.uint8, device=DEV)
    sa = torch.empty((m, k // 32), dtype=torch.uint8, device=DEV)
    sb = torch.empty((n, k // 32), dtype=torch.uint8, device=DEV)
    ops.mx_fill(a, sa, 0, seed, m, k, fmt)
    ops.mx_fill(bt, sb, 1, seed, n, k, fmt)
    return a, sa, bt, sb


def poisoned(m, n):
    # NaN so that an element the kernel skipped cannot match by accident
    return torch.full((m, n), float("nan"), dtype=torch.float32, device=DEV)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_bitwise(c, expected):
    got, want = bits(c), np.ascontiguousarray(expected).view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} element(s) differ, first at "
                           f"{bad[0].tolist()}: got "
                           f"{c[tuple(bad[0])].item()}, want "
                           f"{expected[tuple(bad[0])]}")


def dequant(fmt, codes, scales):
    """float64 value of codes [rows, k] under E8M0 scales [rows, k/32]."""
    return VALUES[fmt][codes] * np.repeat(
        2.0 ** (scales.astype(np.float64) - 127), 32, axis=1)


# ---- the single tile: which lane's scale byte applies where ----

@FMTS
def test_scale_layout_single_tile(fmt):
    """Generator elements, scales drawn independently per (row, k-block)
    from {126, 127, 128, 129}, different for A and B. Bitwise equal to the
    float64 product: every term is a multiple of 1/16 (fp4, two x1/2
    scales on two half-unit values) and the sum stays below 2^20, so the
    fp32 result is exact and unique. A pipe that applied lane l's scale
    byte to other elements than row l & 15, k-block l >> 4 cannot pass."""
    _, ca = reference_elements(fmt, 0, SEED, 16, 128)
    _, cb = reference_elements(fmt, 1, SEED, 128, 16)
    rng = np.random.default_rng(11)
    sa = rng.integers(126, 130, size=(16, 4), dtype=np.uint8)
    sb = rng.integers(126, 130, size=(16, 4), dtype=np.uint8)
    assert not np.array_equal(sa, sb)
    assert len(np.unique(sa)) == 4 and len(np.unique(sb)) == 4
    want = (dequant(fmt, ca, sa) @ dequant(fmt, cb.T, sb).T)
    assert np.array_equal(want, want.astype(np.float32))
    d = ops.mx_gemm16_scaled(dev(pack_codes(fmt, ca)), dev(sa),
                             dev(pack_codes(fmt, cb.T)), dev(sb), fmt)
    assert_bitwise(d, want.astype(np.float32))


def random_codes(fmt, rng, rows, k):
    if fmt == FP4:
        return rng.integers(0, 16, size=(rows, k), dtype=np.uint8)
    finite = np.array([b for b in range(256) if b & 0x7F != 0x7F],
                      dtype=np.uint8)  # no 0x7F / 0xFF (NaN)
    return finite[rng.integers(0, len(finite), size=(rows, k))]


@FMTS
def test_identity_layout_single_tile(fmt):
    """Without the generator: A = [I | 0] with unit scales, Bt random
    finite codes with scales in 120..134 must come back as dequant(Bt)^T
    exactly (each sum has one non-zero term, so the accumulation order
    cannot matter). Then SA non-unit: row i scales by its k-block-0
    factor."""
    rng = np.random.default_rng(12)
    a = np.zeros((16, 128), dtype=np.uint8)
    a[np.arange(16), np.arange(16)] = ONE[fmt]
    bt = random_codes(fmt, rng, 16, 128)
    sb = rng.integers(120, 135, size=(16, 4), dtype=np.uint8)
    assert not np.array_equal(bt[:, :16], bt[:, :16].T)
    b_t = dequant(fmt, bt, sb)[:, :16].T  # [k = i][n]
    for sa in (np.full((16, 4), 127, dtype=np.uint8),
               rng.integers(120, 135, size=(16, 4), dtype=np.uint8)):
        d = ops.mx_gemm16_scaled(dev(pack_codes(fmt, a)), dev(sa),
                                 dev(pack_codes(fmt, bt)), dev(sb), fmt)
        want = b_t * 2.0 ** (sa[:, :1].astype(np.float64) - 127)
        assert np.array_equal(d.cpu().numpy().astype(np.float64), want)


@FMTS
def test_identity_layout_gemm(fmt):
    """The same through the tiled kernel: A = [I | 0] of 128 rows, Bt
    [256, K] random finite codes, SB random in 120..134, first with unit SA,
    then with a non-unit scale per row of A."""
    k = STEP_K[fmt]
    rng = np.random.default_rng(13)
    a = np.zeros((128, k), dtype=np.uint8)
    a[np.arange(128), np.arange(128)] = ONE[fmt]
    bt = random_codes(fmt, rng, 256, k)
    sb = rng.integers(120, 135, size=(256, k // 32), dtype=np.uint8)
    b_t = dequant(fmt, bt, sb)[:, :128].T  # [k = i][n]
    row_scale = rng.integers(120, 135, size=(128, 1), dtype=np.uint8)
    for sa in (np.full((128, k // 32), 127, dtype=np.uint8),
               np.repeat(row_scale, k // 32, axis=1)):
        c = poisoned(128, 256)
        ops.mx_gemm_nt(dev(pack_codes(fmt, a)), dev(sa),
                       dev(pack_codes(fmt, bt)), dev(sb), fmt, out=c)
        want = b_t * 2.0 ** (sa[:, :1].astype(np.float64) - 127)
        assert np.array_equal(c.cpu().numpy().astype(np.float64), want)


# ---- generator fill, GEMM kernel and integer reference ----

@FMTS
@pytest.mark.parametrize("m,n,steps", [(128, 64, 1), (384, 128, 3)])
def test_fill_matches_reference(fmt, m, n, steps):
    k = steps * STEP_K[fmt]
    a, sa, bt, sb = operands(fmt, m, n, k)
    _, ca = reference_elements(fmt, 0, SEED, m, k)
    _, cb = reference_elements(fmt, 1, SEED, k, n)
    assert np.array_equal(a.cpu().numpy(), pack_codes(fmt, ca))
    # Bt[n][k] holds logical B[k][n]
    assert np.array_equal(bt.cpu().numpy(), pack_codes(fmt, cb.T))
    assert np.array_equal(sa.cpu().numpy(),
                          reference_scales(0, SEED, m, k // 32))
    assert np.array_equal(sb.cpu().numpy(),
                          reference_scales(1, SEED, n, k // 32))


@FMTS
@FNS
@pytest.mark.parametrize("m,n,steps", SHAPES)
def test_gemm_exact(fn, fmt, m, n, steps):
    k = steps * STEP_K[fmt]
    c = poisoned(m, n)
    out = fn(*operands(fmt, m, n, k), fmt, out=c)
    assert out.data_ptr() == c.data_ptr()
    assert_bitwise(c, ref_product(fmt, m, n, k))


@FMTS
@FNS
def test_allocating_form(fn, fmt):
    m, n, k = 128, 256, STEP_K[fmt]
    c = fn(*operands(fmt, m, n, k), fmt)
    assert c.shape == (m, n) and c.dtype == torch.float32
    assert_bitwise(c, ref_product(fmt, m, n, k))


@FMTS
@FNS
def test_bound_case(fn, fmt):
    """K = 8192, every scale 128 (x2), every element the most negative:
    fp8 -16 (0xD8) gives (-32)(-32) * 8192 = 2^23, the limit of the
    exactness argument; fp4 code 0xF (-6) gives (-12)(-12) * 8192 =
    1,179,648. Then one element of A changes and only its row moves:
    fp8 A[5][777] = 15 (0x57): 2^23 - 1024 + (30)(-32) = 8386624;
    fp4 A[5][777] = 0.5 (code 1, the high nibble of byte 388):
    1179648 - 144 + (1)(-12) = 1179492."""
    m, n, k = 128, 128, 8192
    kb = k if fmt == FP8 else k // 2
    fill, full = (0xD8, 2.0 ** 23) if fmt == FP8 else (0xFF, 1179648.0)
    a = torch.full((m, kb), fill, dtype=torch.uint8, device=DEV)
    bt = torch.full((n, kb), fill, dtype=torch.uint8, device=DEV)
    sa = torch.full((m, k // 32), 128, dtype=torch.uint8, device=DEV)
    sb = torch.full((n, k // 32), 128, dtype=torch.uint8, device=DEV)
    c = poisoned(m, n)
    fn(a, sa, bt, sb, fmt, out=c)
    assert (bits(c) == np.float32(full).view(np.uint32)).all()
    if fmt == FP8:
        a[5, 777] = 0x57
        moved = 8386624.0
    else:
        a[5, 388] = 0x1F
        moved = 1179492.0
    c = poisoned(m, n)
    fn(a, sa, bt, sb, fmt, out=c)
    want = np.full((m, n), full, dtype=np.float32)
    want[5, :] = moved
    assert np.array_equal(c.cpu().numpy(), want)


@FMTS
def test_where_table(fmt):
    m, n, k = 2048, 2048, STEP_K[fmt]
    where = torch.full((256, 2), -1, dtype=torch.int32, device=DEV)
    c = poisoned(m, n)
    ops.mx_gemm_nt(*operands(fmt, m, n, k), fmt, out=c, where=where)
    assert_bitwise(c, ref_product(fmt, m, n, k))
    w = where.cpu().numpy()
    # every tile wrote its record (a row still at -1/-1 was skipped)
    assert not ((w[:, 0] == -1) & (w[:, 1] == -1)).any()
    xcc = w[:, 0] & 0xF  # XCC id: low 4 bits of the XCC_ID register
    assert ((xcc >= 0) & (xcc <= 7)).all()
    # a CPX-partitioned device has one XCC, so no spread is asserted


# ---- driver ----

def plant(buf, flips):
    """XOR mask into 32-bit element e for every (e, mask)."""
    idx = torch.tensor([e for e, _ in flips], dtype=torch.int64, device=DEV)
    masks = np.array([m for _, m in flips], dtype=np.uint32).view(np.int32)
    flat = buf.view(torch.int32).view(-1)
    flat[idx] = flat[idx] ^ torch.from_numpy(masks).to(DEV)


@FMTS
def test_driver_clean(fmt):
    k = 2 * STEP_K[fmt]
    rep, flops, where = mxgemmtest(256, 256, k, fmt, iters=3, seed=SEED)
    assert rep.clean and rep.first_bad_dword is None and rep.log == []
    assert flops == 3 * 2.0 * 256 * 256 * k
    assert where.shape == (4, 2) and where.dtype == np.int32
    assert not ((where[:, 0] == -1) & (where[:, 1] == -1)).any()


@FMTS
def test_driver_locates_planted_bit(fmt):
    k = 2 * STEP_K[fmt]
    row, col = 200, 77  # tile (1, 0) of the 2 x 2 grid
    index = row * 256 + col
    rep, _, where = mxgemmtest(
        256, 256, k, fmt, iters=2, seed=SEED,
        gold_hook=lambda gold: plant(gold, [(index, 0x00000100)]))
    assert rep.bad_dwords == 2 and rep.bad_bits == 2  # once per iteration
    assert rep.first_bad_dword == index and rep.xor_or == 0x100
    want = int(ref_product(fmt, 256, 256, k)[row, col].view(np.uint32))
    # the log holds (index, gold bits, C bits): gold carries the flip
    assert set(rep.log) == {(index, want ^ 0x100, want)}
    r, c, tile, xcc, hw_id = locate(rep.first_bad_dword, 256, where)
    assert (r, c, tile) == (row, col, 2)
    assert 0 <= xcc <= 7
    assert hw_id == int(where[2][1]) & 0xFFFFFFFF


# ---- argument validation ----

def test_gpu_argument_validation_launches_nothing():
    a, sa, bt, sb = operands(FP8, 128, 128, 128)
    c = poisoned(128, 128)
    with pytest.raises(RuntimeError, match="out must be float32"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=c.to(torch.float64))
    with pytest.raises(RuntimeError, match=r"out must be \[M,N\]"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=poisoned(128, 256))
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=c.cpu())
    with pytest.raises(RuntimeError, match="where must be int32"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=c, where=torch.zeros(
            (1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"int32\[tiles,2\]"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=c, where=torch.zeros(
            (2, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8, out=c,
                       where=torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.mx_gemm_nt(a, sa, bt, sb.cpu(), FP8, out=c)
    with pytest.raises(RuntimeError, match=r"SA \[M, K/32\]"):
        # 128 bytes per row read as fp4 are K = 256: the scales are short
        ops.mx_gemm_nt(a, sa, bt, sb, FP4, out=c)
    with pytest.raises(RuntimeError, match="shape contract"):
        ops.mx_gemm_ref_int(a[:64], sa[:64], bt, sb, FP8, out=c)
    with pytest.raises(RuntimeError, match=r"SA \[M, K/32\]"):
        ops.mx_gemm_nt(a, sa[:, :2].contiguous(), bt, sb, FP8, out=c)
    with pytest.raises(RuntimeError, match="fmt must be"):
        ops.mx_gemm_nt(a, sa, bt, sb, 2, out=c)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.mx_gemm_nt(a, sa, bt, sb, FP8,
                       out=poisoned(128, 129).view(-1)[1:1 + 128 * 128]
                       .view(128, 128))
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.mx_fill(a, sa.cpu(), 0, 0, 128, 128, FP8)
    assert torch.isnan(c).all()  # nothing above may have launched
    before = (a.clone(), sa.clone())
    with pytest.raises(RuntimeError, match="k / 32 bytes"):
        ops.mx_fill(a, sa, 0, 1, 128, 128 * 2, FP4)  # fp4: K = 256 fits a
    assert torch.equal(a, before[0]) and torch.equal(sa, before[1])


# ---- mi-mxgemm ----

def _run_mxgemm(fmt, *extra):
    proc = subprocess.run([str(MI_MXGEMM), "--format", fmt, "--size", "512",
                           "--iters", "4", *extra],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1])


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mi_mxgemm_clean(fmt):
    proc, j = _run_mxgemm(fmt)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert proc.stdout.startswith("mi-mxgemm: ")
    assert f"mxgemmtest selftest: 256x256x256 {fmt} MX product matches the " \
        "host product exactly" in proc.stdout
    assert "mxgemmtest selftest: integer gold matches the host product " \
        "exactly" in proc.stdout
    assert "mxgemmtest selftest: detector caught 3/3 injected flips" \
        in proc.stdout
    assert "spot-check 64/64 vs host" in proc.stdout
    assert j["payload"] == "mi-mxgemmtest" and j["format"] == fmt
    assert (j["m"], j["n"], j["k"], j["iters"]) == (512, 512, 512, 4)
    assert j["compute_clean"] is True
    assert j["bad_elems"] == 0 and j["bad_bits"] == 0
    assert (j["first_bad_row"], j["first_bad_col"], j["first_bad_xcc"]) == \
        (-1, -1, -1)
    assert isinstance(j["tflops"], float) and j["tflops"] > 0
    # the member order log parsers see
    pairs = json.loads(proc.stdout.strip().splitlines()[-1],
                       object_pairs_hook=list)
    assert [key for key, _ in pairs] == [
        "payload", "format", "m", "n", "k", "iters", "tflops",
        "compute_clean", "bad_elems", "bad_bits", "first_bad_row",
        "first_bad_col", "first_bad_xcc", "gold_ms", "max_temp_c",
        "max_power_w"]


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mi_mxgemm_inject(fmt):
    proc, j = _run_mxgemm(fmt, "--inject", "3")
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert j["compute_clean"] is False
    assert j["bad_elems"] == 3 and j["bad_bits"] == 3
    assert (j["first_bad_row"], j["first_bad_col"]) == (0, 0)
    assert 0 <= j["first_bad_xcc"] <= 7
    # flip i sits at element i * (M*N // 3), bit i: one log line each
    elems = [i * (512 * 512 // 3) for i in range(3)]
    want = {(e // 512, e % 512, 1 << i) for i, e in enumerate(elems)}
    pat = re.compile(r"^C\[(\d+)\]\[(\d+)\] expected 0x[0-9a-f]{8} actual "
                     r"0x[0-9a-f]{8} xor 0x([0-9a-f]{8}) xcc (\d) "
                     r"hw_id 0x[0-9a-f]{8}$")
    logged = {(int(mt[1]), int(mt[2]), int(mt[3], 16))
              for mt in map(pat.match, proc.stdout.splitlines()) if mt}
    assert logged == want
