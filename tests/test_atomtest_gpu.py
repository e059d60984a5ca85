"""Global-atomics test on the GPU: every op's result and gold against the
numpy reference, the returning variant's invariants, the lost-update and
planted-flip accounting, ticket and chain mode, the driver and the
mi-atomtest binary.

Shapes are the smallest at which the walk can go wrong: 1 slot (a single
lane), 257 (one tile and a tail lane), 4353 (17 tiles and a tail); W = 9
puts two contributors on one XCD. Every buffer sits inside a larger poisoned
allocation whose guard words are checked."""

import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from k3samd import ops
from k3samd.ops import atomtest as at

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
MI_ATOMTEST = REPO / "native" / "bin" / "mi-atomtest"

DEV = "cuda:0"
SEED = 0xDEADBEEF12345678
SLOTS = [1, 257, 4353]
MAX_SLOTS = max(SLOTS)
W_LIST = [1, 3, 9, 64]
REDUCE_OPS = list(ops.ATOM_REDUCE_OPS)
CHAIN_OPS = list(ops.ATOM_CHAIN_OPS)
GUARD_WORDS = 64           # 256 bytes on either side
POISON = 0x5A5A5A5A
ROUNDS = 3


@functools.lru_cache(maxsize=None)
def ref(op, W, skip=None, seed=SEED):
    """Expected bits of slots 0..4352 (a smaller run is a prefix), computed
    once and shared; read-only."""
    r = at.reference_expected(op, seed, np.arange(MAX_SLOTS, dtype=np.uint64),
                              W, skip=skip)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def ref_init(op, seed=SEED):
    r = at.reference_init(op, seed, np.arange(MAX_SLOTS, dtype=np.uint64))
    r.setflags(write=False)
    return r


def ref_words(op, bits):
    """Bit patterns -> the uint32 words the report counts."""
    if at.slot_bytes(op) == 8:
        return bits.view(np.uint32)  # little endian: low half first
    return bits.astype(np.uint32)


class Guarded:
    """A slot buffer inside a poisoned allocation. `words` is the int32 view
    of everything; `region` the 16-byte-padded part buf_compare takes (its
    padding is poison in every Guarded alike)."""

    def __init__(self, op, slots):
        self.op, self.slots = op, slots
        k = at.slot_bytes(op) // 4
        self.n_words = slots * k
        padded = -(-self.n_words // 4) * 4
        self.words = torch.full((2 * GUARD_WORDS + padded,), POISON,
                                dtype=torch.int32, device=DEV)
        self.region = self.words[GUARD_WORDS:GUARD_WORDS + padded]
        self.buf = self.words[GUARD_WORDS:GUARD_WORDS + self.n_words].view(
            ops.ATOM_OPS[op][0])
        assert self.buf.numel() == slots

    def bits(self):
        return at.tensor_bits(self.op, self.buf)

    def assert_guards_intact(self):
        w = self.words.cpu().numpy().view(np.uint32)
        assert np.all(w[:GUARD_WORDS] == POISON)
        assert np.all(w[GUARD_WORDS + self.n_words:] == POISON)

    def flip(self, word, mask):
        m = mask - (1 << 32) if mask >= 1 << 31 else mask
        self.words[GUARD_WORDS + word] ^= m


def assert_clean(report):
    rep = ops.mem_report_read(report)
    assert rep.clean and rep.first_bad_dword is None
    assert (rep.bad_dwords, rep.bad_bits, rep.xor_or, rep.log) == (0, 0, 0, [])


def assert_flips_reported(rep, flips, want_words):
    """`flips` is a list of (word index, mask) in ascending order."""
    assert rep.bad_dwords == len(flips)
    assert rep.bad_bits == sum(bin(m).count("1") for _, m in flips)
    assert rep.first_bad_dword == flips[0][0]
    xor_or = 0
    for _, m in flips:
        xor_or |= m
    assert rep.xor_or == xor_or
    assert sorted(rep.log) == [
        (g, int(want_words[g]), int(want_words[g]) ^ m) for g, m in flips]


def new_where(rows):
    return torch.full((rows, 2), -1, dtype=torch.int32, device=DEV)


# ---- clean reduce runs ----

@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("op", REDUCE_OPS)
def test_reduce_clean(op, slots):
    buf, gold = Guarded(op, slots), Guarded(op, slots)
    for W in sorted({min(w, at.w_cap(op)) for w in W_LIST}):
        want = ref(op, W)[:slots]
        ops.atom_gold(gold.buf, op, SEED, W)
        assert np.array_equal(gold.bits(), want), (op, W, "gold")
        for rotate in (False, True):
            for returning in (False, True):
                report = ops.mem_report_new(DEV)
                ops.atom_fill(buf.buf, op, SEED)
                if returning:
                    ops.atom_reduce(buf.buf, op, SEED, W, rotate=rotate,
                                    returning=True, gold=gold.buf,
                                    report=report)
                else:
                    ops.atom_reduce(buf.buf, op, SEED, W, rotate=rotate)
                ops.buf_compare(buf.region, gold.region, report)
                assert np.array_equal(buf.bits(), want), (op, W, rotate,
                                                          returning)
                assert_clean(report)
    buf.assert_guards_intact()
    gold.assert_guards_intact()


@pytest.mark.parametrize("op", REDUCE_OPS + CHAIN_OPS)
def test_fill_writes_the_init(op):
    buf = Guarded(op, 257)
    ops.atom_fill(buf.buf, op, SEED)
    assert np.array_equal(buf.bits(), ref_init(op)[:257])
    buf.assert_guards_intact()


# ---- lost update ----

@pytest.mark.parametrize("drop", [(4, 7), (0, 17), (8, 0)])
@pytest.mark.parametrize("op", REDUCE_OPS)
def test_lost_update(op, drop):
    """Workgroup w skips one tile: the result there is the fold without
    contributor w, everything else is untouched, and the compare reports
    exactly the slots whose value depends on that contributor - for add,
    and, or, xor and the float adds these are the slots whose operand is not
    the op's identity (a min / max operand that is not the extreme changes
    nothing, dropped or not)."""
    slots, W = MAX_SLOTS, 9
    w, tile = drop
    buf, gold = Guarded(op, slots), Guarded(op, slots)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    ops.atom_gold(gold.buf, op, SEED, W)
    ops.atom_reduce(buf.buf, op, SEED, W, rotate=True, drop=drop)
    ops.buf_compare(buf.region, gold.region, report)

    full, without = ref(op, W), ref(op, W, skip=w)
    in_tile = np.arange(slots) // ops.ATOM_TILE == tile
    want = np.where(in_tile, without, full)
    assert np.array_equal(buf.bits(), want)
    operand = at.reference_operand(op, SEED, np.arange(slots, dtype=np.uint64),
                                   w, W)
    changed = in_tile & (full != without)
    if at._base(op) in ("add", "and", "or", "xor") or op in (
            "addf32", "addf64", "pkaddbf16", "pkaddf16"):
        assert np.array_equal(changed,
                              in_tile & ~at.identity_operand(op, operand))
        assert changed.any()
    fw, ww = ref_words(op, full), ref_words(op, want)
    bad = np.flatnonzero(fw != ww)
    rep = ops.mem_report_read(report)
    assert rep.bad_dwords == len(bad)
    if len(bad) == 0:
        assert rep.clean
        return
    assert rep.bad_bits == sum(bin(int(a ^ b)).count("1")
                               for a, b in zip(fw[bad], ww[bad]))
    assert rep.first_bad_dword == bad[0]
    triples = {(int(g), int(fw[g]), int(ww[g])) for g in bad}
    assert len(rep.log) == min(len(bad), ops.MEM_LOG_SLOTS)
    assert set(rep.log) <= triples and len(set(rep.log)) == len(rep.log)
    for g, _, _ in rep.log:
        name, slot, _ = at.locate(op, g)
        assert name == op and slot // ops.ATOM_TILE == tile
    buf.assert_guards_intact()


# ---- planted flips ----

@pytest.mark.parametrize("op", ["add", "umin64", "addf32", "maxf64",
                                "pkaddbf16"])
def test_flips_in_the_result_are_accounted_exactly(op):
    slots, W = MAX_SLOTS, 9
    buf, gold = Guarded(op, slots), Guarded(op, slots)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    ops.atom_gold(gold.buf, op, SEED, W)
    ops.atom_reduce(buf.buf, op, SEED, W)
    flips = [(0, 1 << 0), (buf.n_words // 2 + 1, 1 << 17 | 1 << 3),
             (buf.n_words - 1, 1 << 31)]
    for g, m in flips:
        buf.flip(g, m)
    ops.buf_compare(buf.region, gold.region, report)
    assert_flips_reported(ops.mem_report_read(report), flips,
                          ref_words(op, ref(op, W)))


@pytest.mark.parametrize("op", ["or", "and", "or64", "and64"])
def test_flipped_gold_bit_trips_the_returning_invariant(op):
    """`or`: clearing in the gold a bit the init already holds makes every
    returned value violate old & ~final == 0; `and`: setting a bit the init
    lacks violates final & ~old == 0. One report per contributor, each of
    exactly that bit."""
    slots, W, slot = 257, 9, 256
    buf, gold = Guarded(op, slots), Guarded(op, slots)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    ops.atom_gold(gold.buf, op, SEED, W)
    init, final = int(ref_init(op)[slot]), int(ref(op, W)[slot])
    # a bit no operand touches: set (or) / clear (and) from init to final
    stable = (init & final) if op.startswith("or") else \
        (~init & ~final & ((1 << (8 * at.slot_bytes(op))) - 1))
    bit = stable.bit_length() - 1
    word = slot * (at.slot_bytes(op) // 4) + bit // 32
    mask = 1 << (bit % 32)
    gold.flip(word, mask)
    ops.atom_reduce(buf.buf, op, SEED, W, returning=True, gold=gold.buf,
                    report=report)
    rep = ops.mem_report_read(report)
    flipped = int(ref_words(op, ref(op, W))[word]) ^ mask
    assert (rep.bad_dwords, rep.bad_bits, rep.xor_or) == (W, W, mask)
    assert rep.first_bad_dword == word
    assert rep.log == [(word, flipped, flipped ^ mask)] * W
    assert np.array_equal(buf.bits(), ref(op, W)[:slots])  # result unharmed


@pytest.mark.parametrize("op", ["umax", "smin64", "maxf64"])
def test_lowered_gold_trips_the_min_max_invariant(op):
    """A gold below (max) or above (min) every value the slot ever held:
    each of the W returned values violates old <= final / old >= final."""
    slots, W, slot = 257, 9, 3
    buf, gold = Guarded(op, slots), Guarded(op, slots)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    ops.atom_gold(gold.buf, op, SEED, W)
    k = at.slot_bytes(op) // 4
    extreme = {"umax": [0], "smin64": [0xFFFFFFFF, 0x7FFFFFFF],
               "maxf64": [0, 0xFFF00000]}[op]  # 0, INT64_MAX, -inf
    for j, v in enumerate(extreme):
        gold.flip(slot * k + j, int(ref_words(op, ref(op, W))[slot * k + j]) ^ v)
    ops.atom_reduce(buf.buf, op, SEED, W, returning=True, gold=gold.buf,
                    report=report)
    rep = ops.mem_report_read(report)
    assert rep.first_bad_dword is not None
    assert {at.locate(op, g)[1] for g, _, _ in rep.log} == {slot}
    # every contributor reports at least one differing word of that slot
    assert W <= rep.bad_dwords <= W * k
    assert len(rep.log) >= W


# ---- ticket mode ----

DRAWS = 16384


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("C", [1, 8, 64, 1024])
def test_ticket(C, wide):
    report = ops.mem_report_new(DEV)
    cnt, tickets, where = at.run_ticket(DEV, DRAWS, C, wide, report)
    assert_clean(report)
    assert cnt.cpu().tolist() == [DRAWS // C] * C
    t = tickets.cpu().numpy()
    for c in {0, C // 2, C - 1}:
        assert np.array_equal(np.sort(t[c::C]), np.arange(DRAWS // C))
    w = where.cpu().numpy()
    assert w.shape == (DRAWS // 256, 2) and np.all(w[:, 1] != -1)
    assert np.all((w[:, 0] & 0xF) < 8)

    # one ticket overwritten with a duplicate of another of its counter
    c0 = C - 1
    a, b = c0 + 3 * C, c0 + 7 * C
    lost = int(t[a])
    tickets[a] = tickets[b]
    perm = torch.empty(DRAWS, dtype=torch.int32, device=DEV)
    report = ops.mem_report_new(DEV)
    ops.atom_ticket_check(cnt, tickets, perm, report)
    rep = ops.mem_report_read(report)
    index = c0 * (DRAWS // C) + lost
    assert (rep.bad_dwords, rep.first_bad_dword) == (1, index)
    assert rep.log == [(index, lost, 0xFFFFFFFF)]
    assert at.locate_ticket(index, DRAWS, C) == ("ticket", c0, lost)

    # a counter that did not end at n
    tickets[a] = lost
    cnt[c0] += 1
    report = ops.mem_report_new(DEV)
    ops.atom_ticket_check(cnt, tickets, perm, report)
    rep = ops.mem_report_read(report)
    assert rep.log == [(DRAWS + c0, DRAWS // C, DRAWS // C + 1)]
    assert at.locate_ticket(DRAWS + c0, DRAWS, C) == ("counter", c0, None)


def test_ticket_uneven_counters():
    """Draws that are no multiple of the counters: the padding entries of
    the table stay unset and short counters end lower."""
    report = ops.mem_report_new(DEV)
    cnt, tickets, _ = at.run_ticket(DEV, 4353, 64, False, report)
    assert_clean(report)
    assert cnt.cpu().tolist() == [69 if c < 4353 % 64 else 68
                                  for c in range(64)]


# ---- chain mode ----

@pytest.mark.parametrize("op", CHAIN_OPS)
def test_chain_clean_and_flip(op):
    slots = MAX_SLOTS
    k = at.slot_bytes(op) // 4
    idx = np.arange(slots, dtype=np.uint64)
    v = [at.reference_expected(op, SEED, idx, r) for r in range(ROUNDS + 1)]
    assert np.array_equal(v[0], ref_init(op))
    buf = Guarded(op, slots)
    wgs = at.chain_wgs(slots)
    where = new_where(wgs)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    for r in range(ROUNDS):
        ops.atom_chain_round(buf.buf, op, SEED, r, report, where)
        assert np.array_equal(buf.bits(), v[r + 1]), (op, r)
    assert_clean(report)
    w = where.cpu().numpy()
    assert np.all(w[:, 1] != -1) and np.all((w[:, 0] & 0xF) < 8)
    buf.assert_guards_intact()

    # a word flipped between rounds 1 and 2: round 2's returned value
    slot, mask = 4352, 1 << 9
    word = slot * k + (k - 1)
    ops.atom_fill(buf.buf, op, SEED)
    for r in range(2):
        ops.atom_chain_round(buf.buf, op, SEED, r, report, where)
    assert_clean(report)
    buf.flip(word, mask)
    where.fill_(-1)
    ops.atom_chain_round(buf.buf, op, SEED, 2, report, where)
    rep = ops.mem_report_read(report)
    assert_flips_reported(rep, [(word, mask)], ref_words(op, v[2]))
    assert at.locate(op, rep.first_bad_dword) == (op, slot, k - 1)
    xcc_id, hw_id = where[(slot // ops.ATOM_TILE + 2) % wgs].cpu().tolist()
    assert hw_id != -1 and (xcc_id & 0xF) < 8
    after = buf.bits()
    if op.startswith("cas"):  # both compare-and-swaps failed: unchanged
        flipped = ref_words(op, v[2]).copy()
        flipped[word] ^= mask
        want = v[3].copy()
        want[slot] = int(flipped.view(np.uint64)[slot] if k == 2
                         else flipped[slot])
        assert np.array_equal(after, want)
    else:
        assert np.array_equal(after, v[3])


@pytest.mark.parametrize("op", ["cas", "cas64"])
def test_failed_compare_and_swap_leaves_memory_unchanged(op):
    """Round 1 on memory that holds v_0: both the must-fail and the real
    compare-and-swap miss, every slot is reported, nothing is written."""
    slots = 257
    buf = Guarded(op, slots)
    report = ops.mem_report_new(DEV)
    ops.atom_fill(buf.buf, op, SEED)
    ops.atom_chain_round(buf.buf, op, SEED, 1, report, new_where(2))
    assert np.array_equal(buf.bits(), ref_init(op)[:slots])
    rep = ops.mem_report_read(report)
    v0 = ref_words(op, ref_init(op)[:slots])
    v1 = ref_words(op, at.reference_expected(
        op, SEED, np.arange(slots, dtype=np.uint64), 1))
    assert rep.bad_dwords == np.count_nonzero(v0 != v1)
    assert rep.first_bad_dword == np.flatnonzero(v0 != v1)[0]
    for g, expected, actual in rep.log:
        assert (expected, actual) == (int(v1[g]), int(v0[g]))
    buf.assert_guards_intact()


# ---- the driver ----

def test_atomtest_driver():
    res = at.atomtest(DEV, slots=MAX_SLOTS, contributors=9, seed=SEED,
                      ticket_draws=DRAWS, ticket_counters=(8,))
    assert res.clean and res.bad_dwords == 0
    assert list(res.per_op) == REDUCE_OPS
    assert set(res.chain) == set(CHAIN_OPS)
    assert set(res.ticket) == {(32, 8), (64, 8)}
    for name, r in res.per_op.items():
        assert r.report.clean and r.instruction == ops.ATOM_OPS[name][2]
        assert r.ms > 0 and r.gatoms > 0 and r.gbs > 0
    res = at.atomtest(DEV, op_names=["xor64"], slots=257, contributors=3,
                      returning=True, ticket_draws=0, chain_rounds=0)
    assert list(res.per_op) == ["xor64"] and res.clean
    assert not res.ticket and not res.chain


# ---- mi-atomtest ----

def _run_atomtest(*extra):
    proc = subprocess.run(
        [str(MI_ATOMTEST), "--slots", "4353", "--contributors", "9",
         *map(str, extra)], capture_output=True, text=True, timeout=120)
    lines = proc.stdout.strip().splitlines()
    return proc, json.loads(lines[-1]) if lines else None


JSON_KEYS = ["payload", "ops", "slots", "contributors", "iters",
             "atomics_clean", "bad_dwords", "bad_bits", "first_bad_op",
             "first_bad_slot"]


def test_mi_atomtest_clean():
    proc, j = _run_atomtest("--iters", "2")
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "FAIL" not in proc.stdout
    for line in ("26 ops at 4353 slots x 9 contributors match the host "
                 "expectation (device result and device gold)",
                 "lost-update drill reported exactly the dropped tile's "
                 "non-identity slots for every add / and / or / xor op",
                 "detector caught 3/3 planted flips"):
        assert "atomtest selftest: " + line in proc.stdout
    names = REDUCE_OPS + CHAIN_OPS + ["ticket"]
    for p in range(2):
        rows = [ln.split() for ln in proc.stdout.splitlines()
                if ln.split()[:1] == [str(p)]]
        assert [r[1] for r in rows] == names
        for r in rows[:-1]:
            assert r[2] == ops.ATOM_OPS[r[1]][2]
            assert float(r[3]) > 0 and float(r[4]) > 0 and float(r[5]) > 0
    for key in JSON_KEYS + [n + "_gatoms" for n in names]:
        assert key in j, key
    assert j["payload"] == "mi-atomtest" and j["ops"] == names
    assert (j["slots"], j["contributors"], j["iters"]) == (4353, 9, 2)
    assert j["atomics_clean"] is True
    assert (j["bad_dwords"], j["bad_bits"]) == (0, 0)
    assert j["first_bad_op"] is None and j["first_bad_slot"] == -1


def test_mi_atomtest_inject():
    proc, j = _run_atomtest("--iters", "2", "--inject", "3")
    assert proc.returncode == 4, proc.stdout + proc.stderr
    assert "FAIL" not in proc.stdout and "[fault injection ON]" in proc.stdout
    assert j["atomics_clean"] is False
    assert (j["bad_dwords"], j["bad_bits"]) == (3, 3)
    assert (j["first_bad_op"], j["first_bad_slot"]) == ("add", 0)
    bad = sorted(ln for ln in proc.stdout.splitlines()
                 if ln.startswith("bad "))
    want = ref("add", 9, seed=0)  # pass 0 runs seed 0
    expect = sorted(
        "bad add slot %d half 0 expected 0x%08x actual 0x%08x xor 0x%08x"
        % (s, int(want[s]), int(want[s]) ^ (1 << f), 1 << f)
        for f, s in enumerate((0, 1451, 2902)))
    assert bad == expect


def test_mi_atomtest_op_list():
    proc, j = _run_atomtest("--iters", "1", "--ops", "pkaddf16,cas64,ticket")
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert j["ops"] == ["pkaddf16", "cas64", "ticket"]
    assert j["atomics_clean"] is True
