"""Global-atomics test, CPU side: the host code of atom_pattern.h (through
the CPU ops and mi-atomtest's dump) against the independent numpy
reference, order independence of the float ops in their own precision, the
conditions the generator is designed to meet, atom_shape_ok, binding-level
argument checks, the payload's usage errors and the deployment files."""

import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from k3samd import ops
from k3samd.ops import atomtest as at

REPO = Path(__file__).resolve().parent.parent
MI_ATOMTEST = REPO / "native" / "bin" / "mi-atomtest"

SEEDS = [0, 0xDEADBEEF12345678]
ALL_OPS = list(ops.ATOM_OPS)
REDUCE_OPS = list(ops.ATOM_REDUCE_OPS)
INT_OPS = [n for n in REDUCE_OPS if n not in at.FLOAT_OPS]
# around 0, the tile edge and 2^32
EDGE_SLOTS = [0, 1, 255, 256, 257, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
QUALITY_SLOTS = np.arange(4096, dtype=np.uint64)


def w_list(op):
    cap = at.w_cap(op)
    return sorted({w for w in (1, 3, 9, 64) if w <= cap} | {cap})


def _run(*args):
    return subprocess.run([str(MI_ATOMTEST), *map(str, args)],
                          capture_output=True, text=True, timeout=60)


@functools.lru_cache(maxsize=None)
def quality(op, W):
    """(init, expected) over slots 0..4095, computed once and shared."""
    init = at.reference_init(op, SEEDS[1], QUALITY_SLOTS)
    exp = at.reference_expected(op, SEEDS[1], QUALITY_SLOTS, W)
    init.setflags(write=False)
    exp.setflags(write=False)
    return init, exp


# ---- reference agreement ----

def test_op_table_matches_the_header():
    names = ops._C.atom_op_names()
    assert names == ALL_OPS
    assert ALL_OPS[:8] == ["add", "and", "or", "xor", "smin", "smax", "umin",
                           "umax"]
    assert ALL_OPS[8:16] == [n + "64" for n in ALL_OPS[:8]]
    assert ALL_OPS[16:22] == ["addf32", "addf64", "minf64", "maxf64",
                              "pkaddbf16", "pkaddf16"]
    assert tuple(ALL_OPS[22:]) == ops.ATOM_CHAIN_OPS
    assert ops._C.ATOM_REDUCE_OPS == len(REDUCE_OPS) == 22
    for name, (dtype, nbytes, instr, cap) in ops.ATOM_OPS.items():
        assert nbytes == at.slot_bytes(name) == torch.empty(
            0, dtype=dtype).element_size()
        assert instr.startswith("global_atomic_")
        assert cap == at.w_cap(name)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("op", ALL_OPS)
def test_reference_matches_host_ops(op, seed):
    for W in w_list(op):
        init = at.reference_init(op, seed, EDGE_SLOTS)
        exp = at.reference_expected(op, seed, EDGE_SLOTS, W)
        ws = sorted({0, 1, W // 2, W - 1} & set(range(W)))
        opnd = {w: at.reference_operand(op, seed, EDGE_SLOTS, w, W)
                for w in ws}
        for k, slot in enumerate(EDGE_SLOTS):
            assert int(init[k]) == ops.atom_init(op, seed, slot)
            assert int(exp[k]) == ops.atom_expected(op, seed, slot, W)
            for w in ws:
                assert int(opnd[w][k]) == ops.atom_operand(op, seed, slot, w, W)
        assert int(init.max()) < 1 << (8 * at.slot_bytes(op))
        assert int(exp.max()) < 1 << (8 * at.slot_bytes(op))


@pytest.mark.parametrize("slot0", [0, 254, (1 << 32) - 2])
@pytest.mark.parametrize("op", ALL_OPS)
def test_pattern_dump_matches_reference(op, slot0):
    """Runs without a GPU: the dump returns before any HIP call."""
    seed, n = SEEDS[1], 4
    slots = [slot0 + i for i in range(n)]
    for W in w_list(op):
        proc = _run("--pattern-dump", op, seed, W, slot0, n)
        assert proc.returncode == 0, proc.stderr
        lines = proc.stdout.splitlines()
        assert len(lines) == n
        init = at.reference_init(op, seed, slots)
        exp = at.reference_expected(op, seed, slots, W)
        opnd = at.reference_operands(op, seed, slots, W)
        for k, line in enumerate(lines):
            f = line.split()
            assert f[0] == "slot" and int(f[1]) == slots[k]
            assert f[2] == "init" and int(f[3], 16) == int(init[k])
            assert f[4] == "expected" and int(f[5], 16) == int(exp[k])
            assert f[6] == "operands"
            assert [int(v, 16) for v in f[7:]] == [int(v) for v in opnd[:, k]]


def test_chain_values_are_one_sequence():
    """Round r writes what round r + 1 expects to find."""
    for op in ops.ATOM_CHAIN_OPS:
        for slot in (0, 257):
            v = [ops.atom_init(op, 5, slot)] + [
                ops.atom_operand(op, 5, slot, r, 4) for r in range(4)]
            assert len(set(v)) == 5
            for R in range(1, 5):
                assert ops.atom_expected(op, 5, slot, R) == v[R]


# ---- order independence of the float ops ----

def _apply_float(op, start_bits, operand_bits):
    """Sequential application in the op's own precision; returns bits."""
    if op == "addf32":
        acc = np.array([start_bits], dtype=np.uint32).view(np.float32)
        for b in operand_bits:
            acc = acc + np.array([b], dtype=np.uint32).view(np.float32)
        return int(acc.view(np.uint32)[0])
    if op in ("addf64", "minf64", "maxf64"):
        acc = np.array([start_bits], dtype=np.uint64).view(np.float64)
        for b in operand_bits:
            v = np.array([b], dtype=np.uint64).view(np.float64)
            acc = (acc + v if op == "addf64" else
                   np.minimum(acc, v) if op == "minf64" else np.maximum(acc, v))
        return int(acc.view(np.uint64)[0])
    if op == "pkaddf16":
        acc = np.array([start_bits], dtype=np.uint32).view(np.float16)
        for b in operand_bits:
            acc = acc + np.array([b], dtype=np.uint32).view(np.float16)
        assert acc.dtype == np.float16
        return int(acc.view(np.uint32)[0])
    acc = torch.tensor([start_bits], dtype=torch.int64).to(torch.int32) \
        .view(torch.bfloat16)
    for b in operand_bits:
        acc = acc + torch.tensor([b], dtype=torch.int64).to(torch.int32) \
            .view(torch.bfloat16)
    assert acc.dtype == torch.bfloat16
    return int(acc.view(torch.int32)[0]) & 0xFFFFFFFF


def _to_i32_range(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


@pytest.mark.parametrize("op", at.FLOAT_OPS)
def test_float_ops_are_order_independent_at_the_cap(op):
    W = at.w_cap(op)
    rng = np.random.default_rng(12345)
    for slot in (0, 255, 4352):
        init = int(at.reference_init(op, SEEDS[1], [slot])[0])
        operands = [ops.atom_operand(op, SEEDS[1], slot, w, W)
                    for w in range(W)]
        want = ops.atom_expected(op, SEEDS[1], slot, W)
        if op == "pkaddbf16":  # torch.tensor wants values in int32 range
            init = _to_i32_range(init)
            operands = [_to_i32_range(b) for b in operands]
        for _ in range(5):
            order = rng.permutation(W)
            got = _apply_float(op, init, [operands[i] for i in order])
            assert got == want, (op, slot)
    assert ops.atom_shape_ok(op, 4353, W)
    assert not ops.atom_shape_ok(op, 4353, W + 16)


@pytest.mark.parametrize("op", at.FLOAT_OPS)
def test_float_operands_meet_their_rules(op):
    """Integer-valued, never -0, no NaN, min / max never zero, and
    |init| + W * max|operand| within the significand."""
    W = at.w_cap(op)
    slots = QUALITY_SLOTS[:512]
    init = at.reference_init(op, SEEDS[1], slots)
    opnds = [at.reference_operand(op, SEEDS[1], slots, w, W)
             for w in (0, 1, W // 2, W - 1)]

    def values(bits):
        if op == "addf32":
            return [bits.astype(np.uint32).view(np.float32).astype(np.float64)]
        if op in at.PACKED_OPS:
            halves = [(bits & np.uint64(0xFFFF)), (bits >> np.uint64(16))]
            if op == "pkaddf16":
                return [h.astype(np.uint16).view(np.float16).astype(np.float64)
                        for h in halves]
            return [(h.astype(np.uint32) << np.uint32(16)).view(np.float32)
                    .astype(np.float64) for h in halves]
        return [bits.view(np.float64)]

    p = {"addf32": 24, "addf64": 53, "minf64": 53, "maxf64": 53,
         "pkaddbf16": 8, "pkaddf16": 11}[op]
    peak_init = max(np.abs(v).max() for v in values(init))
    peak_op = 0.0
    for bits in [init] + opnds:
        for v in values(bits):
            assert np.all(np.isfinite(v)) and np.all(v == np.round(v))
            assert not np.any(np.signbit(v) & (v == 0))
            if op in ("minf64", "maxf64"):
                assert np.all(v != 0)
    for bits in opnds:
        peak_op = max(peak_op, max(np.abs(v).max() for v in values(bits)))
    if op.startswith(("add", "pkadd")):
        assert peak_init + W * peak_op <= 2.0 ** p


# ---- generator quality: conditions on the generator ----

@pytest.mark.parametrize("op", REDUCE_OPS)
def test_generator_quality(op):
    for W in w_list(op):
        init, exp = quality(op, W)
        distinct = len(np.unique(exp))
        if op in at.PACKED_OPS:
            assert distinct >= 64, (op, W, distinct)
        elif op in INT_OPS:
            assert distinct >= 2048, (op, W, distinct)
        if W >= 2:
            assert np.count_nonzero(exp != init) >= 2048, (op, W)
        if at._base(op) in ("and", "or"):
            ones = np.uint64((1 << (8 * at.slot_bytes(op))) - 1)
            assert not np.any(exp == 0) and not np.any(exp == ones), (op, W)
            assert not np.any(init == 0) and not np.any(init == ones)


@pytest.mark.parametrize("op", ["and", "or", "and64", "or64"])
def test_mask_density_follows_w(op):
    """Bits per operand: half the width at W = 1, then about T / W; every
    non-identity operand changes its slot."""
    bits = 8 * at.slot_bytes(op)
    ones = (1 << bits) - 1
    slots = QUALITY_SLOTS[:256]
    for W in (1, 9, 64):
        count = 0
        acc = at.reference_init(op, 3, slots)
        table = at.reference_operands(op, 3, slots, W)
        for w in range(W):
            v = at.reference_operand(op, 3, slots, w, W)
            assert np.array_equal(table[w], v)
            m = v if op.startswith("or") else v ^ np.uint64(ones)
            count += sum(bin(int(x)).count("1") for x in m)
            nxt = acc | v if op.startswith("or") else acc & v
            assert np.array_equal(nxt != acc, m != 0)
            acc = nxt
        assert count == len(slots) * bits // 2
        assert np.array_equal(acc, at.reference_expected(op, 3, slots, W))


def test_skip_is_the_fold_without_one_contributor():
    for op in REDUCE_OPS:
        W = 9
        slots = QUALITY_SLOTS[:64]
        full = at.reference_expected(op, 1, slots, W)
        without = at.reference_expected(op, 1, slots, W, skip=4)
        operand = at.reference_operand(op, 1, slots, 4, W)
        changed = full != without
        assert not np.any(changed & at.identity_operand(op, operand))
        if at._base(op) in ("add", "and", "or", "xor") or op in (
                "addf32", "addf64", "pkaddbf16", "pkaddf16"):
            assert np.array_equal(changed, ~at.identity_operand(op, operand))
        assert changed.any()


# ---- atom_shape_ok and the bindings' argument checks ----

def test_shape_ok_cases():
    for op in ALL_OPS:
        cap = at.w_cap(op)
        assert cap == (240 if op in at.PACKED_OPS else 4096)
        for slots, W, ok in [(1, 1, True), (4353, 9, True),
                             (1 << 30, cap, True), (0, 1, False),
                             (-1, 1, False), ((1 << 30) + 1, 1, False),
                             (1, 0, False), (1, -3, False),
                             (1, cap + 1, False), (1, cap + 16, False)]:
            assert ops.atom_shape_ok(op, slots, W) is ok, (op, slots, W)
    assert not ops.atom_shape_ok(len(ALL_OPS), 1, 1)
    assert not ops.atom_shape_ok(-1, 1, 1)
    with pytest.raises(ValueError, match="unknown atomics op"):
        ops.atom_op_id("nand")


def test_locate():
    assert at.locate("add", 4352) == ("add", 4352, 0)
    assert at.locate("umin64", 9) == ("umin64", 4, 1)
    assert at.locate("cas64", 8) == ("cas64", 4, 0)
    assert at.locate_ticket(5, 16384, 8) == ("ticket", 0, 5)
    assert at.locate_ticket(2048 * 3 + 7, 16384, 8) == ("ticket", 3, 7)
    assert at.locate_ticket(16384 + 2, 16384, 8) == ("counter", 2, None)


def test_argument_validation_without_a_gpu():
    """Shape and type errors are raised before any device check, so they
    can be exercised on CPU tensors; a correct call then fails only because
    the tensor is not on a GPU."""
    i32 = torch.zeros(257, dtype=torch.int32)
    i64 = torch.zeros(257, dtype=torch.int64)
    report = torch.zeros(ops.MEM_REPORT_LEN, dtype=torch.int64)
    where = torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="unknown atomics op id"):
        ops.atom_fill(i32, 26, 0)
    with pytest.raises(RuntimeError, match="slot size"):
        ops.atom_fill(i32, "add64", 0)
    with pytest.raises(RuntimeError, match="slot size"):
        ops.atom_gold(i64, "addf32", 0, 9)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.atom_fill(i32[::2], "add", 0)
    with pytest.raises(RuntimeError, match="shape contract"):
        ops.atom_fill(i32[:0], "add", 0)
    with pytest.raises(RuntimeError, match="shape contract"):
        ops.atom_gold(i32, "pkaddbf16", 0, 241)
    with pytest.raises(RuntimeError, match="shape contract"):
        ops.atom_reduce(i32, "add", 0, 4097)
    with pytest.raises(RuntimeError, match="must be a reduce op"):
        ops.atom_reduce(i32, "swap", 0, 3)
    with pytest.raises(RuntimeError, match="must be a chain op"):
        ops.atom_chain_round(i32, "add", 0, 0, report, where)
    with pytest.raises(RuntimeError, match="drop must be None"):
        ops.atom_reduce(i32, "add", 0, 3, drop=(3, 0))
    with pytest.raises(RuntimeError, match="drop must be None"):
        ops.atom_reduce(i32, "add", 0, 3, drop=(0, 2))
    with pytest.raises(RuntimeError, match="needs gold and report"):
        ops.atom_reduce(i32, "or", 0, 3, returning=True)
    with pytest.raises(RuntimeError, match="needs gold and report"):
        ops.atom_reduce(i32, "or", 0, 3, gold=i32.clone())
    with pytest.raises(RuntimeError, match="gold must have"):
        ops.atom_reduce(i32, "or", 0, 3, returning=True, gold=i32[:256],
                        report=report)
    with pytest.raises(RuntimeError, match=r"int64\[56\]"):
        ops.atom_reduce(i32, "or", 0, 3, returning=True, gold=i32.clone(),
                        report=report[:55])
    with pytest.raises(RuntimeError, match="round must be in"):
        ops.atom_chain_round(i32, "cas", 0, 4096, report, where)
    with pytest.raises(RuntimeError, match=r"int32\[wgs,2\]"):
        ops.atom_chain_round(i32, "cas", 0, 0, report, where.view(4, 1))
    with pytest.raises(RuntimeError, match="both be int32 or both int64"):
        ops.atom_ticket(i32[:8], i64, where)
    with pytest.raises(RuntimeError, match=r"int32\[ceil\(draws/256\),2\]"):
        ops.atom_ticket(i32[:8], i32, where[:1])
    with pytest.raises(RuntimeError, match="perm must be"):
        ops.atom_ticket_check(i32[:8], i32, i32[:8], report)
    with pytest.raises(RuntimeError, match="0 <= w < W"):
        ops.atom_operand("add", 0, 0, 3, 3)
    with pytest.raises(RuntimeError, match="0 <= w < W"):
        ops.atom_expected("pkaddf16", 0, 0, 241)
    # everything else in order: only the device is missing
    for call in (lambda: ops.atom_fill(i32, "add", 0),
                 lambda: ops.atom_gold(i64, "umax64", 0, 4096),
                 lambda: ops.atom_reduce(i32, "pkaddf16", 0, 240, rotate=True,
                                         drop=(239, 1)),
                 lambda: ops.atom_reduce(i64, "or64", 0, 3, returning=True,
                                         gold=i64.clone(), report=report),
                 lambda: ops.atom_chain_round(i64, "swap64", 0, 4095, report,
                                              where)):
        with pytest.raises(RuntimeError, match="must be on GPU"):
            call()
    with pytest.raises(RuntimeError, match="must be on the same GPU"):
        ops.atom_ticket(i32[:8], i32, where)


# ---- the binary and the deployment files ----

def test_usage_errors_exit_2():
    """Bad arguments are refused before any HIP call."""
    for extra in (["--iters", "2", "--seconds", "2"], ["--iters", "-1"],
                  ["--slots", "0"], ["--slots", str((1 << 30) + 1)],
                  ["--contributors", "0"], ["--contributors", "4097"],
                  ["--ops", "add,nand"], ["--ops", ""], ["--inject", "17"],
                  ["--inject", "0"], ["--inject", "-1"], ["--device", "-1"],
                  ["--inject", "3", "--slots", "2"],
                  ["--inject", "1", "--ops", "swap"],
                  ["--bogus"], ["--iters"], ["--pattern-dump", "add", "0"],
                  ["--pattern-dump", "nand", "0", "1", "0", "1"],
                  ["--pattern-dump", "pkaddf16", "0", "241", "0", "1"],
                  ["--pattern-dump", "add", "0", "1", "0", "0"]):
        proc = _run(*extra)
        assert proc.returncode == 2, (extra, proc.stdout, proc.stderr)
        assert "hip" not in (proc.stdout + proc.stderr).lower(), extra


def test_help_prints_usage():
    proc = _run("--help")
    assert proc.returncode == 0
    for flag in ("--device", "--ops all|LIST", "--slots", "--contributors",
                 "--seconds", "--iters", "--inject",
                 "--pattern-dump OP SEED W SLOT0 N"):
        assert flag in proc.stdout


def test_atomtest_manifest_contract():
    docs = [d for d in yaml.safe_load_all(
        (REPO / "deploy" / "manifests" / "mi-atomtest.yaml").read_text()) if d]
    assert [d["kind"] for d in docs] == ["Job"]
    job = docs[0]
    assert job["metadata"]["name"] == "mi-atomtest"
    assert job["spec"]["backoffLimit"] == 0
    pod = job["spec"]["template"]["spec"]
    assert pod["runtimeClassName"] == "amd"
    assert pod["restartPolicy"] == "Never"
    c = pod["containers"][0]
    assert c["resources"]["limits"]["amd.com/gpu"] == "1"
    assert c["command"] == ["mi-atomtest", "--seconds", "120"]


def test_payload_is_shipped():
    """The binary the manifest runs is in the image and the node install."""
    assert "/src/native/bin/mi-atomtest" in (
        REPO / "deploy" / "docker" / "Dockerfile").read_text()
    assert "mi-atomtest" in (
        REPO / "deploy" / "scripts" / "install-node.sh").read_text()
    assert "$(BIN)/mi-atomtest" in (
        REPO / "native" / "Makefile").read_text()
