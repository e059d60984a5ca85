"""Per-CU self-test on the GPU: the LDS march and the VALU signature against
the numpy oracles, exact accounting of planted corruption, the placement
records and the coverage conditions that validate the HW_ID decode, argument
validation, and the mi-cutest binary.

Shapes are the smallest at which the code can go wrong: one workgroup is
the base case, two and three exercise the cell offset and the `where`
stride; the full-device grid is used only for coverage."""

import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops import cutest as ct
from k3samd.ops.memtest import ADDR, CHECKER, WALK, reference_pattern

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_CUTEST = REPO / "native" / "bin" / "mi-cutest"

DEV = "cuda:0"
SEED = 0xDEADBEEF12345678
CELLS = ops.CU_LDS_CELLS          # 10240
DWORDS = 4 * CELLS                # 40960
# what the LDS holds after phase ph wrote it: (pattern, invert)
PHASE_SPEC = [(ADDR, False), (ADDR, True), (WALK, False), (CHECKER, False)]


@functools.lru_cache(maxsize=None)
def lds_ref(ph, seed, wg):
    """LDS content of workgroup `wg` after phase `ph`, computed once and
    shared; read-only."""
    pattern, invert = PHASE_SPEC[ph]
    r = reference_pattern(pattern, seed, invert, CELLS, cell_offset=wg * CELLS)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def sig_ref(seed, rounds):
    r = ct.reference_signature(seed, rounds)
    r.setflags(write=False)
    return r


def sig_expected(seed, rounds):
    """The ORACLE's signature as the kernel's `expected` operand."""
    return torch.from_numpy(sig_ref(seed, rounds).view(np.int32).copy()).to(DEV)


def new_where(rows):
    return torch.full((rows, 2), -1, dtype=torch.int32, device=DEV)


def assert_raw_clean(report):
    raw = report.cpu().tolist()
    assert raw[2] == -1 and raw[:2] == [0, 0] and not any(raw[3:])
    rep = ops.mem_report_read(report)
    assert rep.clean and rep.first_bad_dword is None
    assert (rep.bad_dwords, rep.bad_bits, rep.xor_or, rep.log) == (0, 0, 0, [])


def check_report(rep, triples_by_g, repeats=1):
    """Exact accounting: `triples_by_g` maps a report dword index to
    (expected, xor_mask)."""
    masks = [m for _, m in triples_by_g.values()]
    triples = {(g, e, e ^ m) for g, (e, m) in triples_by_g.items()}
    assert rep.bad_dwords == repeats * len(masks)
    assert rep.bad_bits == repeats * sum(bin(m).count("1") for m in masks)
    assert rep.first_bad_dword == min(triples_by_g)
    assert rep.xor_or == functools.reduce(lambda a, b: a | b, masks)
    assert not rep.clean
    if repeats * len(masks) <= ops.MEM_LOG_SLOTS:
        assert sorted(rep.log) == sorted(list(triples) * repeats)
    else:
        assert len(rep.log) == ops.MEM_LOG_SLOTS
        assert len(set(rep.log)) == len(rep.log) or repeats > 1
        assert set(rep.log) <= triples


# ---- LDS march ----

@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("stop_after", [0, 1, 2, 3])
def test_lds_dump_matches_reference(stop_after, wgs):
    report, where = ops.mem_report_new(DEV), new_where(wgs)
    dump = torch.full((wgs, DWORDS), 0x5A5A5A5A, dtype=torch.int32,
                      device=DEV)
    ops.cu_lds_march(report, where, SEED, stop_after=stop_after, dump=dump)
    got = dump.cpu().numpy().view(np.uint32).reshape(wgs, CELLS, 4)
    for wg in range(wgs):
        assert np.array_equal(got[wg], lds_ref(stop_after, SEED, wg)), wg
    assert_raw_clean(report)


def test_lds_dump_last_pass_uses_its_own_seed():
    """stop_after applies to the last pass only, whose seed is seed + 1."""
    report, where = ops.mem_report_new(DEV), new_where(2)
    dump = torch.full((2, DWORDS), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ops.cu_lds_march(report, where, 7, passes=2, stop_after=2, dump=dump)
    got = dump.cpu().numpy().view(np.uint32).reshape(2, CELLS, 4)
    for wg in range(2):
        assert np.array_equal(got[wg], lds_ref(2, 8, wg))
    assert_raw_clean(report)


def test_lds_full_march_ends_on_checker():
    report, where = ops.mem_report_new(DEV), new_where(1)
    dump = torch.full((1, DWORDS), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ops.cu_lds_march(report, where, SEED, dump=dump)
    got = dump.cpu().numpy().view(np.uint32).reshape(CELLS, 4)
    assert np.array_equal(got, lds_ref(3, SEED, 0))
    assert_raw_clean(report)


@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("passes", [1, 2])
def test_lds_clean_march(passes, wgs):
    report, where = ops.mem_report_new(DEV), new_where(wgs)
    ops.cu_lds_march(report, where, SEED, passes=passes)
    assert_raw_clean(report)


def lds_flips():
    """(wg, lds_dword, mask) on three workgroups: the first and the last
    dword of the LDS, one dword in each of the four 64-thread read groups
    (cell & 255 in 0..63, 64..127, 128..191, 192..255; every k), and one in
    workgroup 2."""
    return [(0, 0, 0x00000001), (0, DWORDS - 1, 0x80000000),
            (0, 4 * 5 + 1, 0x00010100), (0, 4 * (70 + 256) + 2, 0xFFFFFFFF),
            (0, 4 * (130 + 512) + 3, 0x00000400),
            (0, 4 * (200 + 256 * 39) + 0, 0x40000002),
            (2, 4 * 777 + 1, 0x00800000)]


def lds_triples(flips, ph, seed):
    return {wg * DWORDS + d:
            (int(lds_ref(ph, seed, wg).reshape(-1)[d]), m)
            for wg, d, m in flips}


@pytest.mark.parametrize("ph", [0, 1, 2, 3])
def test_lds_planted_corruption(ph):
    """A flip planted after phase ph's write is found by phase ph + 1's
    verify, against the pattern of the phase it was planted in."""
    report, where = ops.mem_report_new(DEV), new_where(3)
    flips = lds_flips()
    ops.cu_lds_march(report, where, SEED,
                     inject=[(wg, d, m, ph) for wg, d, m in flips])
    check_report(ops.mem_report_read(report), lds_triples(flips, ph, SEED))


def test_lds_planted_corruption_overflows_log():
    flips = [(i % 3, (i * (DWORDS - 1)) // 39,
              (0x9E3779B1 * (i + 1)) & 0xFFFFFFFF) for i in range(40)]
    assert len({(wg, d) for wg, d, _ in flips}) == 40
    report, where = ops.mem_report_new(DEV), new_where(3)
    ops.cu_lds_march(report, where, SEED,
                     inject=[(wg, d, m, 1) for wg, d, m in flips])
    check_report(ops.mem_report_read(report), lds_triples(flips, 1, SEED))


def test_lds_inject_is_pass_0_only_and_second_pass_is_clean():
    """Two passes: the flip is planted (and found) in pass 0 alone."""
    report, where = ops.mem_report_new(DEV), new_where(1)
    ops.cu_lds_march(report, where, 3, passes=2, inject=[(0, 9, 0x10, 2)])
    check_report(ops.mem_report_read(report), lds_triples([(0, 9, 0x10)], 2, 3))


def test_lds_report_accumulates():
    report, where = ops.mem_report_new(DEV), new_where(3)
    flips = lds_flips()
    inject = [(wg, d, m, 0) for wg, d, m in flips]
    ops.cu_lds_march(report, where, SEED, inject=inject)
    ops.cu_lds_march(report, where, SEED, inject=inject)
    check_report(ops.mem_report_read(report), lds_triples(flips, 0, SEED),
                 repeats=2)


# ---- VALU signature ----

def run_signature(wgs, seed, rounds, expected=None, inject=None,
                  want_out=True):
    report, where = ops.mem_report_new(DEV), new_where(4 * wgs)
    out = (torch.full((256 * wgs, 4), 0x5A5A5A5A, dtype=torch.int32,
                      device=DEV) if want_out else None)
    ops.cu_valu_signature(report, where, seed, rounds,
                          sig_expected(seed, rounds)
                          if expected is None else expected,
                          sig_out=out, inject=inject)
    got = None if out is None else \
        out.cpu().numpy().view(np.uint32).reshape(4 * wgs, 64, 4)
    return report, where.cpu().numpy(), got


@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("rounds", [1, 7, 64])
def test_signature_matches_oracle(rounds, wgs):
    report, _, got = run_signature(wgs, SEED, rounds)
    want = sig_ref(SEED, rounds)
    for w in range(4 * wgs):
        bad = np.argwhere(got[w] != want)
        assert bad.size == 0, (w, bad[:4].tolist())
    assert_raw_clean(report)  # the LDS fold agrees too


def test_signature_seed_zero_and_no_sig_out():
    report, _, got = run_signature(2, 0, 7, want_out=False)
    assert got is None
    assert_raw_clean(report)


def valu_g(wg, wave, lane, k):
    c = (wg * 4 + wave) * 64 + lane
    return 4 * (ops.CU_FOLD_CELL_BIT | c) if k == 4 else 4 * c + k


def test_signature_injects_are_accounted_exactly():
    """Lane 0, lane 63, every datapath k (4 = the LDS fold), wave 3, and a
    workgroup other than 0."""
    rounds = 7
    want = sig_ref(SEED, rounds)
    inject = [(0, 0, 0, 0, 0x00000001), (0, 1, 63, 1, 0x80000000),
              (0, 2, 17, 2, 0x00010100), (0, 3, 63, 3, 0xFFFFFFFF),
              (2, 3, 0, 3, 0x00000400), (1, 0, 40, 4, 0x00200000),
              (2, 3, 63, 4, 0x00000002)]
    triples = {}
    for wg, wave, lane, k, m in inject:
        e = ct.reference_fold(want[lane, 3]) if k == 4 else int(want[lane, k])
        triples[valu_g(wg, wave, lane, k)] = (e, m)
    report, _, got = run_signature(3, SEED, rounds, inject=inject)
    check_report(ops.mem_report_read(report), triples)
    # sig_out holds the cells as compared: the oracle with the flips in
    expect_out = np.broadcast_to(want, (12, 64, 4)).copy()
    for wg, wave, lane, k, m in inject:
        if k < 4:
            expect_out[wg * 4 + wave, lane, k] ^= np.uint32(m)
    assert np.array_equal(got, expect_out)
    for g, (e, m) in triples.items():
        loc = ct.locate(g, "valu")
        assert valu_g(loc["wg"], loc["wave"], loc["lane"], loc["k"]) == g


@pytest.mark.parametrize("wgs", [1, 3])
def test_signature_wrong_expected_reports_every_cell(wgs):
    """`expected` of another seed: every differing dword of every wave is
    counted (all 64 x 4 of them per wave, plus the folds) and the log stays
    bounded."""
    rounds = 7
    mine, other = sig_ref(SEED, rounds), sig_ref(SEED + 1, rounds)
    diff = mine ^ other
    assert (diff != 0).all()  # every one of the 64 x 4 dwords differs
    fold_diff = [ct.reference_fold(a) ^ ct.reference_fold(b)
                 for a, b in zip(mine[:, 3], other[:, 3])]
    assert all(fold_diff)
    report, _, _ = run_signature(wgs, SEED, rounds,
                                 expected=sig_expected(SEED + 1, rounds))
    rep = ops.mem_report_read(report)
    waves = 4 * wgs
    assert rep.bad_dwords == waves * (64 * 4 + 64)
    bits = sum(bin(int(v)).count("1") for v in diff.reshape(-1)) \
        + sum(bin(v).count("1") for v in fold_diff)
    assert rep.bad_bits == waves * bits
    assert rep.first_bad_dword == 0
    assert len(rep.log) == ops.MEM_LOG_SLOTS
    for g, expected, actual in rep.log:
        loc = ct.locate(g, "valu")
        if loc["k"] == 4:
            assert expected == ct.reference_fold(other[loc["lane"], 3])
            assert actual == ct.reference_fold(mine[loc["lane"], 3])
        else:
            assert expected == int(other[loc["lane"], loc["k"]])
            assert actual == int(mine[loc["lane"], loc["k"]])


# ---- placement ----

def test_where_is_fully_written():
    report, lw = ops.mem_report_new(DEV), new_where(3)
    ops.cu_lds_march(report, lw, SEED)
    lw = lw.cpu().numpy()
    assert not ((lw[:, 0] == -1) & (lw[:, 1] == -1)).any()
    assert ((lw[:, 0] & 0xF) < 8).all()
    _, vw, _ = run_signature(3, SEED, 1)
    assert vw.shape == (12, 2)
    assert not ((vw[:, 0] == -1) & (vw[:, 1] == -1)).any()
    assert ((vw[:, 0] & 0xF) < 8).all()
    for wg in range(3):
        rows = vw[4 * wg:4 * wg + 4]
        keys = {ct.cu_key(x, h) for x, h in rows.tolist()}
        simds = {ct.decode_hw_id(h)["simd"] for _, h in rows.tolist()}
        assert len(keys) == 1, (wg, rows.tolist())  # one CU per workgroup
        assert simds == {0, 1, 2, 3}, (wg, rows.tolist())


@functools.lru_cache(maxsize=None)
def whole_device():
    """One driver run over the whole device, shared."""
    return ct.cutest(DEV, seed=1, passes=1, rounds=16, max_launches=8)


def histogram(cov):
    """Per-key row counts, decoded, for the assertion messages."""
    return sorted((tuple(ct.describe_key(k).values()), n)
                  for k, n in cov.per_key.items())


def test_driver_covers_every_cu_and_simd():
    """One resident workgroup per CU forces full coverage on an idle card:
    a condition on the HW_ID decode and the dispatch, not a measurement."""
    res = whole_device()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert res["cus_total"] == cus
    assert res["lds"].clean and res["valu"].clean
    assert res["miscompares"] == []
    assert 1 <= res["launches"] <= 8
    lds_cov, valu_cov = res["lds_coverage"], res["valu_coverage"]
    print("launches", res["launches"], "lds keys", len(lds_cov.keys),
          "valu keys", len(valu_cov.keys), "simds", len(valu_cov.simds))
    # never more distinct keys than CUs: the key carries no field that
    # varies inside one CU
    assert len(lds_cov.keys) <= cus, histogram(lds_cov)
    assert len(valu_cov.keys) <= cus, histogram(valu_cov)
    # and every CU / SIMD reached within the cap
    assert res["cus_covered"] == cus, histogram(lds_cov)
    assert len(valu_cov.keys) == cus, histogram(valu_cov)
    assert res["simds_covered"] == 4 * cus, histogram(valu_cov)
    assert res["covered"] is True
    assert lds_cov.keys == valu_cov.keys
    # rows recorded: 4 x CUs workgroups per launch (x 4 waves for VALU)
    assert sum(lds_cov.per_key.values()) == res["launches"] * 4 * cus
    assert sum(valu_cov.per_key.values()) == res["launches"] * 16 * cus


def test_driver_reports_decoded_miscompares(monkeypatch):
    """A wrong `expected` through the driver: every logged miscompare comes
    back with a decoded location."""
    real = ops.cu_signature_expected
    monkeypatch.setattr(ops, "cu_signature_expected",
                        lambda seed, rounds: real(seed + 1, rounds))
    res = ct.cutest(DEV, seed=1, passes=1, rounds=4, max_launches=1)
    assert res["lds"].clean and not res["valu"].clean
    assert len(res["miscompares"]) == ops.MEM_LOG_SLOTS
    for m in res["miscompares"]:
        assert m["kind"] == "valu"
        assert set(m) >= {"wg", "wave", "lane", "k", "xcc", "se", "sh", "cu",
                          "simd", "expected", "actual"}
        assert 0 <= m["xcc"] < 8 and 0 <= m["simd"] < 4


# ---- validation ----

def test_rejected_calls_launch_nothing():
    report, good = ops.mem_report_new(DEV), new_where(4)
    before = report.clone()
    exp = sig_expected(SEED, 1)
    march, sig = ops.cu_lds_march, ops.cu_valu_signature
    with pytest.raises(RuntimeError, match="report must be int64"):
        march(report.to(torch.int32), good, 0)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        march(report[:-1], good, 0)
    with pytest.raises(RuntimeError, match="where must be int32"):
        march(report, good.to(torch.int64), 0)
    with pytest.raises(RuntimeError, match=r"int32\[wgs,2\]"):
        march(report, good[:0], 0)
    with pytest.raises(RuntimeError, match=r"int32\[4\*wgs,2\]"):
        sig(report, good[:3], 0, 1, exp)
    with pytest.raises(RuntimeError, match="passes must be >= 1"):
        march(report, good, 0, passes=0)
    with pytest.raises(RuntimeError, match="stop_after must be 0..4"):
        march(report, good, 0, stop_after=5)
    with pytest.raises(RuntimeError, match="rounds must be >= 1"):
        sig(report, good, 0, 0, exp)
    for row in [(4, 0, 1, 0), (0, DWORDS, 1, 0), (0, 0, 1, 4), (-1, 0, 1, 0),
                (0, 0, 1 << 32, 0)]:
        with pytest.raises(RuntimeError, match="inject row out of range"):
            march(report, good, 0, inject=[row])
    for row in [(1, 0, 0, 0, 1), (0, 4, 0, 0, 1), (0, 0, 64, 0, 1),
                (0, 0, 0, 5, 1), (0, 0, 0, 0, 1 << 32)]:
        with pytest.raises(RuntimeError, match="inject row out of range"):
            sig(report, good, 0, 1, exp, inject=[row])
    with pytest.raises(RuntimeError, match=r"int32\[wgs,40960\]"):
        march(report, good, 0, dump=torch.zeros((3, DWORDS), dtype=torch.int32,
                                                device=DEV))
    with pytest.raises(RuntimeError, match=r"int32\[256\*wgs,4\]"):
        sig(report, good, 0, 1, exp, sig_out=torch.zeros(
            (255, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match=r"int32\[64,4\]"):
        sig(report, good, 0, 1, exp[:63])
    with pytest.raises(RuntimeError, match="where must be on GPU"):
        march(report, good.cpu(), 0)
    with pytest.raises(RuntimeError, match="same GPU"):
        march(report.cpu(), good, 0)
    with pytest.raises(RuntimeError, match="same GPU"):
        march(report, good, 0, dump=torch.zeros((4, DWORDS),
                                                dtype=torch.int32))
    with pytest.raises(RuntimeError, match="expected must be on the same GPU"):
        sig(report, good, 0, 1, exp.cpu())
    with pytest.raises(ValueError, match="4 entries"):
        march(report, good, 0, inject=[(0, 0, 1)])
    # nothing above may have launched: report and where are untouched
    assert torch.equal(report, before)
    assert (good == -1).all()


# ---- mi-cutest ----

def _run_cutest(*extra):
    proc = subprocess.run([str(MI_CUTEST), "--passes", "2", "--rounds", "64",
                           *extra],
                          capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1])


def test_mi_cutest_clean():
    proc, j = _run_cutest("--iters", "2")
    assert proc.returncode == 0, proc.stdout + proc.stderr
    for line in ("device signature of one workgroup (4 waves, 64 rounds) "
                 "matches the host signature",
                 "LDS detector caught 3/3 planted flips",
                 "VALU detector caught 3/3 planted flips"):
        assert "cutest selftest: " + line in proc.stdout
    assert j["payload"] == "mi-cutest"
    assert j["cu_clean"] is True and j["lds_clean"] is True
    assert j["valu_clean"] is True
    assert j["cus_total"] == \
        torch.cuda.get_device_properties(0).multi_processor_count
    assert j["cus_covered"] == j["cus_total"]
    assert j["simds_covered"] == 4 * j["cus_total"]
    assert j["lds_bytes_per_cu"] == 163840
    assert j["launches"] == 2 and j["bad_dwords"] == 0


def test_mi_cutest_inject():
    proc, j = _run_cutest("--iters", "2", "--inject", "3")
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert j["cu_clean"] is False
    assert j["bad_dwords"] == 3
    assert j["lds_bad_dwords"] == 2 and j["valu_bad_dwords"] == 1
    assert j["lds_bad_bits"] + j["valu_bad_bits"] == 3
    located = [ln for ln in proc.stdout.splitlines() if ln.startswith("bad ")]
    assert len(located) == 3
    for ln in located:
        words = ln.split()
        for name in ("xcc", "se", "sh", "cu", "simd", "expected", "actual",
                     "xor"):
            assert name in words, ln
    assert sum(" byte 0x" in ln for ln in located) == 2
    assert sum(" lane " in ln and " datapath " in ln for ln in located) == 1
