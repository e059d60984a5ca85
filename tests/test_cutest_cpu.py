"""Per-CU self-test, CPU side: the host VALU signature (mi-cutest's dump,
compiled from cu_pattern.h) against the independent numpy / Fraction
oracle, the ranges and the diffusion the derivation relies on, the HW_ID
decode, coverage and locate helpers, binding-level argument checks, the
payload's usage errors and the Job manifest."""

import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops import cutest as ct

REPO = Path(__file__).resolve().parent.parent
MI_CUTEST = REPO / "native" / "bin" / "mi-cutest"

SEEDS = [0, 0xDEADBEEF12345678]
ROUNDS = [1, 7, 64]


def _run(*args):
    return subprocess.run([str(MI_CUTEST), *map(str, args)],
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_signature_dump_matches_reference(seed, rounds):
    """Runs without a GPU: the dump returns before any HIP call."""
    proc = _run("--signature-dump", seed, rounds)
    assert proc.returncode == 0, proc.stderr
    got = np.array([[int(w, 16) for w in line.split()]
                    for line in proc.stdout.splitlines()], dtype=np.uint32)
    assert got.shape == (64, 4)
    want = ct.reference_signature(seed, rounds)
    assert want.dtype == np.uint32 and want.shape == (64, 4)
    assert np.array_equal(got, want)


def test_signature_depends_on_seed_rounds_and_lane():
    a = ct.reference_signature(0, 7)
    assert (a != ct.reference_signature(1, 7)).all()
    assert (a != ct.reference_signature(1 << 32, 7)).all()  # high seed word
    assert (a != ct.reference_signature(0, 8)).all()
    for k in range(4):
        assert len(set(a[:, k].tolist())) == 64  # no two lanes agree


def test_chains_stay_in_range():
    """f and d start in [1, 2) and stay in [1, 8) for 4096 rounds: no
    denormal, infinity or NaN can occur, which the bitwise comparison
    relies on. 8 lanes' worth of fp64 would do, all 64 are checked."""
    for i, (f, d, _) in enumerate(ct.signature_chains(SEEDS[1], 4096)):
        d = np.array(d)
        hi = 2.0 if i == 0 else 8.0
        assert f.dtype == np.float32
        assert (f >= 1.0).all() and (f < hi).all(), i
        assert (d >= 1.0).all() and (d < hi).all(), i
    assert i == 4096


def test_fp32_recipe_is_fmaf_at_a_rounding_case():
    """The float64 expression rounds once, like fmaf: with f = 1 + 2^-23,
    a = 0.5 + 4 * 2^-24 and b = 1 the exact sum is 1.5 + 2.5 * 2^-23 + 2^-45,
    just above a tie, so the fused result is 1.5 + 3 * 2^-23; rounding the
    product first loses the 2^-45 and the tie then goes to even, 1.5 +
    2 * 2^-23."""
    f = np.float32(1 + 2.0 ** -23)
    a = np.float32(0.5 + 4 * 2.0 ** -24)
    b = np.float32(1.0)
    fused = np.float32(np.float64(f) * np.float64(a) + np.float64(b))
    split = np.float32(np.float32(f * a) + b)
    assert fused == np.float32(1.5 + 3 * 2.0 ** -23)
    assert split == np.float32(1.5 + 2 * 2.0 ** -23)


def test_every_exchange_distance_and_full_diffusion():
    """Rounds 0..5 use the six distances 1, 2, 4, 8, 16, 32, so a change in
    one lane's starting integer reaches all 64 d3 within 6 rounds — and not
    sooner."""
    assert {1 << (r % 6) for r in range(6)} == {1, 2, 4, 8, 16, 32}
    base = list(ct.signature_chains(5, 6))
    for lane in (0, 37, 63):
        other = list(ct.signature_chains(5, 6, perturb=(lane, 0x00010000)))
        reached = [sum(x != y for x, y in zip(b[2], o[2]))
                   for b, o in zip(base, other)]
        assert reached == [1, 2, 4, 8, 16, 32, 64], (lane, reached)
        # the float chains never see the integer chain
        assert np.array_equal(base[6][0], other[6][0])
        assert base[6][1] == other[6][1]
    full = ct.reference_signature(5, 6, perturb=(37, 0x00010000))
    ref = ct.reference_signature(5, 6)
    assert (full[:, 3] != ref[:, 3]).all()
    assert np.array_equal(full[:, :3], ref[:, :3])


def _hw(wave=0, simd=0, pipe=0, cu=0, sh=0, se=0, tg=0, vm=0, queue=0,
        state=0, me=0):
    return (wave | simd << 4 | pipe << 6 | cu << 8 | sh << 12 | se << 13
            | tg << 16 | vm << 20 | queue << 24 | state << 27 | me << 30)


def test_decode_hw_id_and_cu_key():
    fields = dict(wave=9, simd=2, pipe=1, cu=11, sh=1, se=5, tg=7, vm=3,
                  queue=6, state=4, me=2)
    word = _hw(**fields)
    assert ct.decode_hw_id(word) == fields
    assert ct.decode_hw_id(word - (1 << 32)) == fields  # as a signed int32
    base = ct.cu_key(3, word)
    assert ct.describe_key(base) == {"xcc": 3, "se": 5, "sh": 1, "cu": 11}
    # fields that vary inside one CU must not change the key
    for name, value in (("wave", 0), ("simd", 0), ("pipe", 3), ("tg", 0),
                        ("vm", 15), ("queue", 0), ("state", 0), ("me", 0)):
        assert ct.cu_key(3, _hw(**{**fields, name: value})) == base, name
    # fields that name the CU must
    for name, value in (("cu", 10), ("sh", 0), ("se", 4)):
        assert ct.cu_key(3, _hw(**{**fields, name: value})) != base, name
    assert ct.cu_key(2, word) != base
    assert ct.cu_key(3 | 0x50, word) == base  # only XCC_ID[3:0] counts
    # distinct (xcc, se, sh, cu) give distinct keys
    keys = {ct.cu_key(x, _hw(cu=c, sh=h, se=s)) for x in range(8)
            for s in range(8) for h in range(2) for c in range(16)}
    assert len(keys) == 8 * 8 * 2 * 16


def _table(n_xcc, n_se, n_cu, waves=4):
    rows = []
    for x in range(n_xcc):
        for s in range(n_se):
            for c in range(n_cu):
                for w in range(waves):
                    rows.append((x, _hw(wave=w, simd=w, cu=c, se=s, vm=5)))
    return np.array(rows, dtype=np.int64)


def test_coverage_on_synthetic_tables():
    full = _table(8, 4, 8)
    cov = ct.coverage(full)
    assert len(cov.keys) == 256 and len(cov.simds) == 1024
    assert set(cov.per_key.values()) == {4}
    # one CU missing
    missing = full[~((full[:, 0] == 3)
                     & (((full[:, 1] >> 8) & 0xFF) == ((2 << 5) | 7)))]
    cov = ct.coverage(missing)
    assert len(cov.keys) == 255 and len(cov.simds) == 1020
    assert ct.cu_key(3, _hw(cu=7, se=2)) not in cov.keys
    # duplicates: the same rows twice count once, the histogram doubles
    cov = ct.coverage(np.concatenate([full, full]))
    assert len(cov.keys) == 256 and len(cov.simds) == 1024
    assert set(cov.per_key.values()) == {8}
    # a SIMD never seen shows in the pair count alone
    cov = ct.coverage(_table(8, 4, 8, waves=3))
    assert len(cov.keys) == 256 and len(cov.simds) == 768
    # int32 tables with the sign bit set (ME_ID = 2 or 3) decode alike
    signed = np.array([[1, _hw(simd=3, cu=2, se=1, me=3) - (1 << 32)]],
                      dtype=np.int32)
    cov = ct.coverage(signed)
    assert cov.keys == {ct.cu_key(1, _hw(cu=2, se=1))}
    assert cov.simds == {(ct.cu_key(1, _hw(cu=2, se=1)), 3)}
    merged = ct.Coverage()
    merged.update(ct.coverage(missing))
    merged.update(ct.coverage(full))
    assert len(merged.keys) == 256
    assert sorted(set(merged.per_key.values())) == [4, 8]


def test_locate_round_trips():
    per_wg = ops.CU_LDS_BYTES // 4
    assert per_wg == 40960
    assert ct.locate(0, "lds") == {"wg": 0, "byte": 0, "cell": 0, "k": 0}
    assert ct.locate(per_wg - 1, "lds") == {"wg": 0, "byte": 163836,
                                            "cell": 10239, "k": 3}
    assert ct.locate(per_wg, "lds") == {"wg": 1, "byte": 0, "cell": 0, "k": 0}
    assert ct.locate(5 * per_wg + 4 * 777 + 2, "lds") == {
        "wg": 5, "byte": 16 * 777 + 8, "cell": 777, "k": 2}
    for wg, wave, lane, k in [(0, 0, 0, 0), (0, 3, 63, 3), (1, 0, 0, 0),
                              (1023, 3, 63, 3), (7, 2, 33, 1)]:
        c = (wg * 4 + wave) * 64 + lane
        assert ct.locate(4 * c + k, "valu") == {"wg": wg, "wave": wave,
                                                "lane": lane, "k": k}
        assert ct.locate(4 * (ops.CU_FOLD_CELL_BIT | c), "valu") == {
            "wg": wg, "wave": wave, "lane": lane, "k": 4}
    with pytest.raises(ValueError):
        ct.locate(0, "hbm")


def test_reference_fold():
    assert ct.reference_fold(0) == 0
    assert ct.reference_fold(1) == 0b11110
    assert ct.reference_fold(0x80000000) == 0b1111
    assert ct.reference_fold(0xFFFFFFFF) == 0


def test_constants():
    assert (ops.CU_LDS_BYTES, ops.CU_LDS_CELLS, ops.CU_WG_THREADS,
            ops.CU_WAVES) == (163840, 10240, 256, 4)
    assert ops.CU_LDS_CELLS % ops.CU_WG_THREADS == 0  # no ragged tail
    if ops.native_available():
        from k3samd import _C
        assert (_C.CU_LDS_BYTES, _C.CU_LDS_CELLS, _C.CU_WG_THREADS,
                _C.CU_WAVES) == (163840, 10240, 256, 4)


@pytest.mark.parametrize("rounds", ROUNDS + [256])
@pytest.mark.parametrize("seed", SEEDS)
def test_cu_signature_expected_matches_oracle(seed, rounds):
    if not ops.native_available():
        pytest.skip("native extension not built")
    got = ops.cu_signature_expected(seed, rounds)
    assert got.dtype == torch.int32 and tuple(got.shape) == (64, 4)
    assert not got.is_cuda
    assert np.array_equal(got.numpy().view(np.uint32),
                          ct.reference_signature(seed, rounds))


def test_early_argument_validation():
    """Binding checks fire before any launch, so they work without a GPU."""
    if not ops.native_available():
        pytest.skip("native extension not built")
    report = torch.zeros(ops.MEM_REPORT_LEN, dtype=torch.int64)
    where = torch.zeros((4, 2), dtype=torch.int32)
    exp = ops.cu_signature_expected(0, 1)
    march, sig = ops.cu_lds_march, ops.cu_valu_signature
    with pytest.raises(RuntimeError, match="rounds must be >= 1"):
        ops.cu_signature_expected(0, 0)
    with pytest.raises(RuntimeError, match="report must be int64"):
        march(report.to(torch.int32), where, 0)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        sig(report[:-1], where, 0, 1, exp)
    with pytest.raises(RuntimeError, match="where must be int32"):
        march(report, where.to(torch.int64), 0)
    with pytest.raises(RuntimeError, match=r"int32\[wgs,2\]"):
        march(report, torch.zeros((4, 3), dtype=torch.int32), 0)
    with pytest.raises(RuntimeError, match=r"int32\[wgs,2\]"):
        march(report, torch.zeros((8, 2), dtype=torch.int32)[::2], 0)
    with pytest.raises(RuntimeError, match=r"int32\[4\*wgs,2\]"):
        sig(report, torch.zeros((6, 2), dtype=torch.int32), 0, 1, exp)
    with pytest.raises(RuntimeError, match="passes must be >= 1"):
        march(report, where, 0, passes=0)
    for bad in (-1, 5):
        with pytest.raises(RuntimeError, match="stop_after must be 0..4"):
            march(report, where, 0, stop_after=bad)
    with pytest.raises(RuntimeError, match="rounds must be >= 1"):
        sig(report, where, 0, 0, exp)
    with pytest.raises(RuntimeError, match=r"int32\[64,4\]"):
        sig(report, where, 0, 1, exp.to(torch.int64))
    with pytest.raises(RuntimeError, match="inject row out of range"):
        march(report, where, 0, inject=[(0, 0, 1, 0), (4, 0, 1, 0)])
    with pytest.raises(RuntimeError, match="inject row out of range"):
        march(report, where, 0, inject=[(0, 40960, 1, 0)])
    with pytest.raises(RuntimeError, match="inject row out of range"):
        sig(report, where, 0, 1, exp, inject=[(0, 0, 64, 0, 1)])
    with pytest.raises(RuntimeError, match=r"int64\[n,4\], n <= 256"):
        march(report, where, 0, inject=[(0, 0, 1, 0)] * 257)
    with pytest.raises(ValueError, match="5 entries"):
        sig(report, where, 0, 1, exp, inject=[(0, 0, 0, 0)])
    with pytest.raises(RuntimeError, match=r"int32\[wgs,40960\]"):
        march(report, where, 0, dump=torch.zeros((4, 40959),
                                                 dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"int32\[256\*wgs,4\]"):
        sig(report, where, 0, 1, exp, sig_out=torch.zeros((256, 4)))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        sig(report, where, 0, 1, exp, sig_out=torch.zeros(
            256 * 4 + 4, dtype=torch.int32)[1:-3].view(256, 4))
    # everything else in order: only the device is missing
    with pytest.raises(RuntimeError, match="where must be on GPU"):
        march(report, where, 0, inject=[(3, 40959, 0xFFFFFFFF, 3)],
              dump=torch.zeros((4, 40960), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="where must be on GPU"):
        sig(report, where, 0, 1, exp, inject=[(0, 3, 63, 4, 0xFFFFFFFF)],
            sig_out=torch.zeros((256, 4), dtype=torch.int32))


def test_usage_errors_exit_2():
    """Bad arguments are refused before any HIP call."""
    for extra in (["--iters", "2", "--seconds", "2"], ["--iters", "-1"],
                  ["--passes", "0"], ["--rounds", "0"], ["--inject", "17"],
                  ["--inject", "0"], ["--inject", "-1"], ["--device", "-1"],
                  ["--bogus"], ["--iters"], ["--signature-dump", "0"],
                  ["--signature-dump", "0", "0"]):
        proc = _run(*extra)
        assert proc.returncode == 2, (extra, proc.stdout, proc.stderr)


def test_help_prints_usage():
    proc = _run("--help")
    assert proc.returncode == 0
    for flag in ("--device", "--seconds", "--iters", "--passes", "--rounds",
                 "--inject", "--signature-dump SEED ROUNDS"):
        assert flag in proc.stdout


def test_cutest_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-cutest.yaml").read_text()) if d]
    assert [d["kind"] for d in docs] == ["Job"]
    job = docs[0]
    assert job["metadata"]["name"] == "mi-cutest"
    assert job["spec"]["backoffLimit"] == 0
    pod = job["spec"]["template"]["spec"]
    assert pod["runtimeClassName"] == "amd"
    assert pod["restartPolicy"] == "Never"
    c = pod["containers"][0]
    assert c["resources"]["limits"]["amd.com/gpu"] == "1"
    assert c["command"] == ["mi-cutest", "--seconds", "120"]


def test_payload_is_shipped():
    """The binary the manifest runs is in the image and the node install."""
    assert "/src/native/bin/mi-cutest" in (
        REPO / "deploy" / "docker" / "Dockerfile").read_text()
    assert "mi-cutest" in (
        REPO / "deploy" / "scripts" / "install-node.sh").read_text()
