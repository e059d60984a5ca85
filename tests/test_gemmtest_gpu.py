"""Verified bf16 MFMA GEMM on the GPU: the MFMA kernel and the integer
reference kernel, each bitwise against the numpy product; layout and
general-data checks independent of the generator; the `where` table; exact
accounting of the compare kernel; the driver and mi-stream --gemmtest.

Shapes are the smallest at which the kernels can still go wrong: one tile
with one, two and an odd number of K-steps, two tiles along either axis,
a non-square non-power-of-two grid, and 256 blocks."""

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
SHAPES = [(128, 128, 64), (128, 128, 128), (128, 128, 192), (256, 128, 64),
          (128, 256, 64), (384, 640, 320), (2048, 2048, 64)]


@functools.lru_cache(maxsize=None)
def ref_product(m, n, k):
    """Reference computed once per shape and shared; returned read-only."""
    r = reference_product(SEED, m, n, k)
    r.setflags(write=False)
    return r


def operands(m, n, k, seed=SEED):
    a = torch.empty((m, k), dtype=torch.bfloat16, device=DEV)
    bt = torch.empty((n, k), dtype=torch.bfloat16, device=DEV)
    ops.gemm_fill(a, 0, seed, m, k)
    ops.gemm_fill(bt, 1, seed, n, k)
    return a, bt


def poisoned(m, n):
    # NaN so that an element the kernel skipped cannot match by accident
    return torch.full((m, n), float("nan"), dtype=torch.float32, device=DEV)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_bitwise(c, expected):
    got, want = bits(c), expected.view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} element(s) differ, first at "
                           f"{bad[0].tolist()}: got "
                           f"{c[tuple(bad[0])].item()}, want "
                           f"{expected[tuple(bad[0])]}")


@pytest.mark.parametrize("m,n,k", [(128, 64, 64), (384, 128, 320)])
def test_fill_matches_reference(m, n, k):
    a, bt = operands(m, n, k)
    assert np.array_equal(a.float().cpu().numpy(),
                          reference_operand(0, SEED, m, k).astype(np.float32))
    # Bt[n][k] holds logical B[k][n]
    assert np.array_equal(bt.float().cpu().numpy(),
                          reference_operand(1, SEED, k, n).T.astype(np.float32))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_mfma_gemm_exact(m, n, k):
    a, bt = operands(m, n, k)
    c = poisoned(m, n)
    out = ops.gemm_bf16_nt(a, bt, out=c)
    assert out.data_ptr() == c.data_ptr()
    assert_bitwise(c, ref_product(m, n, k))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_ref_int_exact(m, n, k):
    a, bt = operands(m, n, k)
    gold = poisoned(m, n)
    ops.gemm_ref_int(a, bt, out=gold)
    assert_bitwise(gold, ref_product(m, n, k))


def test_allocating_form():
    m, n, k = 128, 256, 64
    a, bt = operands(m, n, k)
    for fn in (ops.gemm_bf16_nt, ops.gemm_ref_int):
        c = fn(a, bt)
        assert c.shape == (m, n) and c.dtype == torch.float32
        assert_bitwise(c, ref_product(m, n, k))


@pytest.mark.parametrize("fn", [ops.gemm_bf16_nt, ops.gemm_ref_int],
                         ids=["mfma", "ref_int"])
def test_bound_case(fn):
    """K = 32768 with every operand -16: each sum reaches 2^23, the limit
    of the exactness argument. Then one element of A becomes 15 and only
    its row changes: 2^23 - (-16)(-16) + 15*(-16) = 8388112."""
    m, n, k = 128, 128, 32768
    a = torch.full((m, k), -16.0, dtype=torch.bfloat16, device=DEV)
    bt = torch.full((n, k), -16.0, dtype=torch.bfloat16, device=DEV)
    c = poisoned(m, n)
    fn(a, bt, out=c)
    assert (bits(c) == np.float32(2 ** 23).view(np.uint32)).all()
    a[5, 777] = 15.0
    c = poisoned(m, n)
    fn(a, bt, out=c)
    got = c.cpu().numpy()
    want = np.full((m, n), 2.0 ** 23, dtype=np.float32)
    want[5, :] = 8388112.0
    assert np.array_equal(got, want)


def test_identity_layout():
    """Layout check independent of the generator: A = I with an
    asymmetric random Bt must reproduce Bt transposed, exactly."""
    g = torch.Generator().manual_seed(1)
    a = torch.eye(128, dtype=torch.bfloat16, device=DEV)
    bt = torch.randn(256, 128, generator=g).to(torch.bfloat16).to(DEV)
    c = poisoned(128, 256)
    ops.gemm_bf16_nt(a, bt, out=c)
    assert torch.equal(c, bt.T.float())


def test_general_data():
    """Random normal bf16 against a float64 product. Bound: the standard
    gamma_K accumulation bound |C - C64| <= K*u*(|A|.|B|) with
    u = 2^-23 (which allows a truncating adder), 1 % slack for the
    higher-order terms: derived, not tuned."""
    m, n, k = 256, 384, 512
    g = torch.Generator().manual_seed(2)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    bt = torch.randn(n, k, generator=g).to(torch.bfloat16)
    c = poisoned(m, n)
    ops.gemm_bf16_nt(a.to(DEV), bt.to(DEV), out=c)
    a64, b64 = a.double().numpy(), bt.double().numpy().T
    c64 = a64 @ b64
    bound = 1.01 * k * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64))
    err = np.abs(c.cpu().numpy().astype(np.float64) - c64)
    print(f"max err {err.max():.3e}, max err/bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


def test_where_table():
    m, n, k = 2048, 2048, 64
    a, bt = operands(m, n, k)
    where = torch.full((256, 2), -1, dtype=torch.int32, device=DEV)
    c = poisoned(m, n)
    ops.gemm_bf16_nt(a, bt, out=c, where=where)
    assert_bitwise(c, ref_product(m, n, k))
    w = where.cpu().numpy()
    # every tile wrote its record (a row still at -1/-1 was skipped)
    assert not ((w[:, 0] == -1) & (w[:, 1] == -1)).any()
    xcc = w[:, 0] & 0xF  # XCC id: low 4 bits of the XCC_ID register
    assert ((xcc >= 0) & (xcc <= 7)).all()
    # a CPX-partitioned device has one XCC, so no spread is asserted


# ---- buf_compare: the same exact accounting as the memtest verify ----

N_ELEMS = 384 * 640


def gold_and_copy():
    gold = torch.from_numpy(ref_product(384, 640, 320).copy()).to(DEV)
    return gold, gold.clone()


def plant(buf, flips):
    """XOR mask into 32-bit element e for every (e, mask)."""
    idx = torch.tensor([e for e, _ in flips], dtype=torch.int64, device=DEV)
    masks = np.array([m for _, m in flips], dtype=np.uint32).view(np.int32)
    flat = buf.view(torch.int32).view(-1)
    flat[idx] = flat[idx] ^ torch.from_numpy(masks).to(DEV)


def standard_flips():
    """Element 0, the last element, mid-matrix, and both sides of a wave
    (64 cells = 256 elements) and of a block (256 cells = 1024 elements)
    boundary."""
    return sorted({0: 0x00000001, N_ELEMS - 1: 0x80000000,
                   N_ELEMS // 2 + 2: 0x00010100, 255: 0xFFFFFFFF,
                   256: 0x00000400, 1023: 0x00200000,
                   1024: 0x40000000}.items())


def many_flips(count=40):
    last = N_ELEMS - 1
    es = sorted({0, last} | {(i * last) // (count - 1) for i in range(count)})
    assert len(es) == count
    return [(e, (0x9E3779B1 * (i + 1)) & 0xFFFFFFFF or 1)
            for i, e in enumerate(es)]


def check_report(rep, flips, gold, calls=1):
    """Exact accounting of planted corruption (as the memtest GPU test)."""
    flat = bits(gold).reshape(-1)
    triples = {(e, int(flat[e]), int(flat[e]) ^ m) for e, m in flips}
    assert rep.bad_dwords == calls * len(flips)
    assert rep.bad_bits == calls * sum(bin(m).count("1") for _, m in flips)
    assert rep.first_bad_dword == min(e for e, _ in flips)
    assert rep.xor_or == functools.reduce(lambda a, b: a | b,
                                          (m for _, m in flips))
    assert not rep.clean
    if calls * len(flips) <= ops.MEM_LOG_SLOTS:
        assert len(rep.log) == calls * len(flips)
        assert set(rep.log) == triples
    else:
        assert len(rep.log) == ops.MEM_LOG_SLOTS
        assert set(rep.log) <= triples


def test_compare_clean_leaves_report_untouched():
    gold, c = gold_and_copy()
    report = ops.mem_report_new(DEV)
    ops.buf_compare(c, gold, report)
    raw = report.cpu().tolist()
    assert raw[2] == -1 and raw[:2] == [0, 0] and not any(raw[3:])
    rep = ops.mem_report_read(report)
    assert rep.clean and rep.first_bad_dword is None and rep.log == []


def test_compare_planted_flips():
    gold, c = gold_and_copy()
    flips = standard_flips()
    plant(c, flips)
    report = ops.mem_report_new(DEV)
    ops.buf_compare(c, gold, report)
    check_report(ops.mem_report_read(report), flips, gold)


def test_compare_log_is_capped():
    gold, c = gold_and_copy()
    flips = many_flips()
    plant(c, flips)
    report = ops.mem_report_new(DEV)
    ops.buf_compare(c, gold, report)
    check_report(ops.mem_report_read(report), flips, gold)


def test_compare_report_accumulates():
    gold, c = gold_and_copy()
    flips = standard_flips()
    plant(c, flips)
    report = ops.mem_report_new(DEV)
    ops.buf_compare(c, gold, report)
    ops.buf_compare(c, gold, report)
    check_report(ops.mem_report_read(report), flips, gold, calls=2)


def test_compare_small_and_ragged():
    """One cell, and a region that ends inside a wave."""
    for n in (4, 4 * 65):
        gold = torch.arange(n, dtype=torch.float32, device=DEV)
        c = gold.clone()
        plant(c, [(n - 1, 0x8)])
        report = ops.mem_report_new(DEV)
        ops.buf_compare(c, gold, report)
        rep = ops.mem_report_read(report)
        assert (rep.bad_dwords, rep.bad_bits, rep.first_bad_dword) == \
            (1, 1, n - 1)


# ---- driver ----

def test_gemmtest_driver_clean():
    rep, flops, where = gemmtest(256, 256, 128, iters=3, seed=SEED)
    assert rep.clean and rep.first_bad_dword is None and rep.log == []
    assert flops == 3 * 2.0 * 256 * 256 * 128
    assert where.shape == (4, 2) and where.dtype == np.int32
    assert not ((where[:, 0] == -1) & (where[:, 1] == -1)).any()


def test_gemmtest_driver_locates_planted_bit():
    row, col = 200, 77  # tile (1, 0) of the 2 x 2 grid
    index = row * 256 + col
    rep, _, where = gemmtest(
        256, 256, 128, iters=2, seed=SEED,
        gold_hook=lambda gold: plant(gold, [(index, 0x00000100)]))
    assert rep.bad_dwords == 2 and rep.bad_bits == 2  # once per iteration
    assert rep.first_bad_dword == index and rep.xor_or == 0x100
    want = int(ref_product(256, 256, 128)[row, col].view(np.uint32))
    # the log holds (index, gold bits, C bits): gold carries the flip
    assert set(rep.log) == {(index, want ^ 0x100, want)}
    r, c, tile, xcc, hw_id = locate(rep.first_bad_dword, 256, where)
    assert (r, c, tile) == (row, col, 2)
    assert 0 <= xcc <= 7
    assert hw_id == int(where[2][1]) & 0xFFFFFFFF


def test_gpu_argument_validation_launches_nothing():
    a, bt = operands(128, 128, 64)
    c = poisoned(128, 128)
    with pytest.raises(RuntimeError, match="out must be float32"):
        ops.gemm_bf16_nt(a, bt, out=c.to(torch.float64))
    with pytest.raises(RuntimeError, match=r"out must be \[M,N\]"):
        ops.gemm_bf16_nt(a, bt, out=poisoned(128, 256))
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.gemm_bf16_nt(a, bt, out=c.cpu())
    with pytest.raises(RuntimeError, match="where must be int32"):
        ops.gemm_bf16_nt(a, bt, out=c, where=torch.zeros(
            (1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"int32\[tiles,2\]"):
        ops.gemm_bf16_nt(a, bt, out=c, where=torch.zeros(
            (2, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="same GPU"):
        ops.gemm_bf16_nt(a, bt, out=c,
                         where=torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="must be on GPU"):
        ops.gemm_bf16_nt(a, bt.cpu(), out=c)
    with pytest.raises(RuntimeError, match="shape contract"):
        ops.gemm_ref_int(a[:64], bt, out=c)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.gemm_bf16_nt(a, bt, out=poisoned(128, 129).view(-1)[1:1 + 128 * 128]
                         .view(128, 128))
    report = ops.mem_report_new(DEV)
    with pytest.raises(RuntimeError, match="same byte size"):
        ops.buf_compare(c, c[:64], report)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        ops.buf_compare(c, c.clone(), report[:-1])
    # nothing above may have launched: the output is still all poison
    assert torch.isnan(c).all()
    assert ops.mem_report_read(report).clean


# ---- mi-stream --gemmtest ----

def _run_gemmtest(*extra):
    proc = subprocess.run([str(MI_STREAM), "--gemmtest", "--gemm-size", "512",
                           "--gemm-iters", "4", *extra],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1])


def test_mi_stream_gemmtest_clean():
    proc, j = _run_gemmtest()
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "gemmtest selftest: 256x256x128 MFMA product and integer gold " \
        "match the host product exactly" in proc.stdout
    assert "gemmtest selftest: detector caught 3/3 injected flips" \
        in proc.stdout
    assert "spot-check 64/64 vs host" in proc.stdout
    assert j["payload"] == "mi-gemmtest"
    assert (j["m"], j["n"], j["k"], j["iters"]) == (512, 512, 512, 4)
    assert j["compute_clean"] is True
    assert j["bad_elems"] == 0 and j["bad_bits"] == 0
    assert (j["first_bad_row"], j["first_bad_col"], j["first_bad_xcc"]) == \
        (-1, -1, -1)
    # the member order log parsers see
    pairs = json.loads(proc.stdout.strip().splitlines()[-1],
                       object_pairs_hook=list)
    assert [key for key, _ in pairs] == [
        "payload", "m", "n", "k", "iters", "bad_elems", "bad_bits",
        "first_bad_row", "first_bad_col", "first_bad_xcc", "avg_tflops",
        "gold_ms", "max_temp_c", "max_power_w", "compute_clean"]


def test_mi_stream_gemmtest_inject():
    proc, j = _run_gemmtest("--gemm-inject", "3")
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
