"""Global-atomics integrity test: the independent numpy reference of the
generator, the decode of a report index, and the driver.

``reference_init`` / ``reference_operand`` / ``reference_expected``
re-derive ``hip/atom_pattern.h`` without sharing its code:

* the hash in wrap-around uint64 numpy arithmetic over a whole array of
  slots;
* add / xor / min / max as a fold over the contributors in the op's own
  width (uint32 / int32 / uint64 / int64 arrays);
* and / or not as a fold but from the rule behind it: every token belongs
  to exactly one contributor below W, so the result is the init with every
  token bit (but those of a skipped contributor) set or cleared;
* floats as int64 sums, minima and maxima converted once by numpy
  (``astype(float32)``, ``astype(float16)``, the high half of a float32 for
  bf16) instead of the header's integer encoder.

``atomtest`` runs fill -> gold -> reduce -> compare for every op, then the
ticket and the chain phase, and returns per-op reports and rates.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from k3samd import ops

_U64 = (1 << 64) - 1
_C_SLOT = 0x9E3779B97F4A7C15
_C_IDX = 0xC2B2AE3D27D4EB4F
_C_OP = 0x165667B19E3779F9
_IDX_LAYOUT = 1 << 40
_IDX_TOKEN = 1 << 41

INT_BASES = ("add", "and", "or", "xor", "smin", "smax", "umin", "umax")
FLOAT_OPS = ("addf32", "addf64", "minf64", "maxf64", "pkaddbf16", "pkaddf16")
PACKED_OPS = ("pkaddbf16", "pkaddf16")


def _u(v):
    return np.uint64(int(v) & _U64)


def op_name(op) -> str:
    return op if isinstance(op, str) else list(ops.ATOM_OPS)[int(op)]


def slot_bytes(op) -> int:
    return 8 if op_name(op).endswith("64") else 4


def w_cap(op) -> int:
    return (ops.ATOM_MAX_PACKED if op_name(op) in PACKED_OPS
            else ops.ATOM_MAX_CONTRIBUTORS)


def _slots(slots):
    return np.atleast_1d(np.asarray(slots, dtype=np.uint64))


def _mix(op, seed, slots, i):
    """h(op, seed, slot, i) over an array of slots."""
    k = ((int(i) + 1) * _C_IDX) ^ ((ops.atom_op_id(op) + 1) * _C_OP) ^ int(seed)
    x = (slots * _u(_C_SLOT)) ^ _u(k)
    x = x ^ (x >> _u(30))
    x = x * _u(0xBF58476D1CE4E5B9)
    x = x ^ (x >> _u(27))
    x = x * _u(0x94D049BB133111EB)
    return x ^ (x >> _u(31))


def _trunc(op, v):
    return v if slot_bytes(op) == 8 else v & _u(0xFFFFFFFF)


def _base(op):
    name = op_name(op)
    return name[:-2] if name.endswith("64") else name


# ---- and / or ----

def _tokens(op, seed, slots, W):
    """(r bit, r2 bit, [token bit], [token owner]) as uint64 arrays."""
    bits = 8 * slot_bytes(op)
    h = _mix(op, seed, slots, _IDX_LAYOUT)
    r = h & _u(bits - 1)
    r2 = (r + _u(1)) & _u(bits - 1)
    s = (h >> _u(32)) % _u(bits - 2)
    tok, owner = [], []
    for j in range(bits // 2):
        pos = (s + _u(7 * j)) % _u(bits - 2)
        tok.append(_u(1) << ((r + _u(2) + pos) & _u(bits - 1)))
        hj = _mix(op, seed, slots, _IDX_TOKEN + j)
        owner.append(((hj >> _u(32)) * _u(W)) >> _u(32))
    return _u(1) << r, _u(1) << r2, tok, owner


def _bit_init(op, seed, slots):
    rbit, r2bit, tok, _ = _tokens(op, seed, slots, 1)
    union = np.zeros_like(slots)
    for t in tok:
        union = union | t
    h = _mix(op, seed, slots, 0)
    if _base(op) == "or":
        return _trunc(op, (h & ~union & ~rbit) | r2bit)
    return _trunc(op, (h | union | rbit) & ~r2bit)


def _bit_mask(op, seed, slots, W, keep):
    """OR of the token bits whose owner satisfies keep(owner)."""
    _, _, tok, owner = _tokens(op, seed, slots, W)
    m = np.zeros_like(slots)
    for t, o in zip(tok, owner):
        m = m | np.where(keep(o), t, _u(0))
    return m


# ---- floats ----

def _float_int(op, seed, slots, i):
    """The integer behind a float value, int64."""
    h = _mix(op, seed, slots, i)
    name = op_name(op)
    if name == "addf32":
        hi = (h >> _u(32)).astype(np.int64)
        return hi % 2097153 - 1048576 if i == 0 else hi % 2049 - 1024
    if name == "addf64":
        if i == 0:
            return (h >> _u(23)).astype(np.int64) - (1 << 40)
        return (h >> _u(33)).astype(np.int64) - (1 << 30)
    return (h.view(np.int64) >> np.int64(12)) | np.int64(1)


def _packed_int(op, seed, slots, i, k):
    f = ((_mix(op, seed, slots, i) >> _u(16 * k)) & _u(0xFFFF)).astype(np.int64)
    if op_name(op) == "pkaddbf16":
        return f % 33 - 16 if i == 0 else np.where(f & 1, 1, -1)
    return f % 257 - 128 if i == 0 else f % 17 - 8


def _half_bits(op, v):
    if op_name(op) == "pkaddbf16":
        return (v.astype(np.float32).view(np.uint32) >> np.uint32(16)) \
            .astype(np.uint64)
    return v.astype(np.float16).view(np.uint16).astype(np.uint64)


def _packed_bits(op, lo, hi):
    return _half_bits(op, lo) | (_half_bits(op, hi) << _u(16))


def _float_bits(op, v):
    if op_name(op) == "addf32":
        return v.astype(np.float32).view(np.uint32).astype(np.uint64)
    return v.astype(np.float64).view(np.uint64)


# ---- the three functions, over arrays of slots ----

def reference_init(op, seed, slots):
    """uint64 array: the bits every slot of `slots` holds before any
    atomic."""
    slots = _slots(slots)
    name = op_name(op)
    if name in PACKED_OPS:
        return _packed_bits(op, _packed_int(op, seed, slots, 0, 0),
                            _packed_int(op, seed, slots, 0, 1))
    if name in FLOAT_OPS:
        return _float_bits(op, _float_int(op, seed, slots, 0))
    if _base(op) in ("and", "or"):
        return _bit_init(op, seed, slots)
    return _trunc(op, _mix(op, seed, slots, 0))


def reference_operand(op, seed, slots, w, W):
    """uint64 array: the bits contributor `w` of `W` applies (chain ops:
    the value round `w` writes)."""
    slots = _slots(slots)
    name = op_name(op)
    if name in PACKED_OPS:
        return _packed_bits(op, _packed_int(op, seed, slots, w + 1, 0),
                            _packed_int(op, seed, slots, w + 1, 1))
    if name in FLOAT_OPS:
        return _float_bits(op, _float_int(op, seed, slots, w + 1))
    if _base(op) in ("and", "or"):
        m = _bit_mask(op, seed, slots, W, lambda o: o == _u(w))
        return _trunc(op, m if _base(op) == "or" else ~m)
    return _trunc(op, _mix(op, seed, slots, w + 1))


def reference_operands(op, seed, slots, W):
    """uint64 [W, len(slots)]: every contributor's operand. The and / or
    tokens are laid out once instead of once per contributor."""
    slots = _slots(slots)
    if _base(op) not in ("and", "or") or op_name(op) in FLOAT_OPS:
        return np.stack([reference_operand(op, seed, slots, w, W)
                         for w in range(int(W))])
    _, _, tok, owner = _tokens(op, seed, slots, W)
    m = np.zeros((int(W), len(slots)), dtype=np.uint64)
    col = np.arange(len(slots))
    for t, o in zip(tok, owner):
        m[o.astype(np.int64), col] |= t  # one owner per token and slot
    return _trunc(op, m if _base(op) == "or" else ~m)


def _typed(op, bits):
    """The bit patterns in the integer type the op compares in."""
    wide = slot_bytes(op) == 8
    if _base(op) in ("smin", "smax"):
        return bits.view(np.int64) if wide else \
            bits.astype(np.uint32).view(np.int32)
    return bits if wide else bits.astype(np.uint32)


def _untyped(v):
    if v.dtype in (np.int64, np.uint64):
        return v.view(np.uint64)
    return v.view(np.uint32).astype(np.uint64)


def reference_expected(op, seed, slots, W, skip=None):
    """uint64 array: the bits after all W contributors but `skip`."""
    slots = _slots(slots)
    name = op_name(op)
    todo = [w for w in range(int(W)) if w != skip]
    if name in ops.ATOM_CHAIN_OPS:
        return _trunc(op, _mix(op, seed, slots, W))
    if name in PACKED_OPS:
        lo = _packed_int(op, seed, slots, 0, 0)
        hi = _packed_int(op, seed, slots, 0, 1)
        for w in todo:
            lo = lo + _packed_int(op, seed, slots, w + 1, 0)
            hi = hi + _packed_int(op, seed, slots, w + 1, 1)
        return _packed_bits(op, lo, hi)
    if name in FLOAT_OPS:
        acc = _float_int(op, seed, slots, 0)
        for w in todo:
            v = _float_int(op, seed, slots, w + 1)
            acc = (np.minimum(acc, v) if name == "minf64" else
                   np.maximum(acc, v) if name == "maxf64" else acc + v)
        return _float_bits(op, acc)
    base = _base(op)
    if base in ("and", "or"):
        skipped = _u(_U64 if skip is None else skip)
        m = _bit_mask(op, seed, slots, W, lambda o: o != skipped)
        init = _bit_init(op, seed, slots)
        return _trunc(op, init | m if base == "or" else init & ~m)
    acc = _typed(op, reference_init(op, seed, slots))
    for w in todo:
        v = _typed(op, _trunc(op, _mix(op, seed, slots, w + 1)))
        if base == "add":
            acc = acc + v
        elif base == "xor":
            acc = acc ^ v
        elif base in ("smin", "umin"):
            acc = np.minimum(acc, v)
        else:
            acc = np.maximum(acc, v)
    return _untyped(acc)


def identity_operand(op, operand_bits):
    """Boolean array: the operand can never change a slot."""
    name = op_name(op)
    ones = _u(_U64 if slot_bytes(op) == 8 else 0xFFFFFFFF)
    if name in ("minf64", "maxf64"):
        return np.zeros(operand_bits.shape, dtype=bool)
    base = _base(op)
    if base in ("and", "umin"):
        return operand_bits == ones
    if base == "smin":
        return operand_bits == ones >> _u(1)
    if base == "smax":
        return operand_bits == (ones ^ (ones >> _u(1)))
    return operand_bits == _u(0)


def bits_to_numpy(op, bits):
    """The uint64 bit patterns as an array of the slot's width (uint32 or
    uint64)."""
    return bits.astype(np.uint32) if slot_bytes(op) == 4 else bits


def locate(op, dword):
    """A report dword index of a reduce or chain op -> (op name, slot, half):
    half 0 is the low (or only) 32 bits of the slot."""
    if slot_bytes(op) == 8:
        return op_name(op), int(dword) // 2, int(dword) % 2
    return op_name(op), int(dword), 0


def locate_ticket(dword, draws, counters):
    """A report dword index of atom_ticket_check -> ("ticket", counter,
    ticket) or ("counter", counter, None)."""
    row = -(-int(draws) // int(counters))
    d = int(dword)
    if d < counters * row:
        return "ticket", d // row, d % row
    return "counter", d - counters * row, None


# ---- device helpers ----

def slot_buffer(op, slots, device):
    """(storage, view): a zeroed tensor of the op's dtype padded to whole
    16-byte cells (what buf_compare takes) and its first `slots` elements."""
    import torch

    dtype, nbytes = ops.ATOM_OPS[op_name(op)][:2]
    per_cell = 16 // nbytes
    padded = -(-int(slots) // per_cell) * per_cell
    storage = torch.zeros(padded, dtype=dtype, device=device)
    return storage, storage[:int(slots)]


def tensor_bits(op, t):
    """A slot tensor's content as a uint64 numpy array of bit patterns."""
    import torch

    raw = t.detach().cpu().contiguous()
    if slot_bytes(op) == 8:
        return raw.view(torch.int64).numpy().view(np.uint64).copy()
    return raw.view(torch.int32).numpy().view(np.uint32).astype(np.uint64)


def chain_wgs(slots) -> int:
    """Workgroups of a chain launch: one per tile, at most 1024."""
    return min(-(-int(slots) // ops.ATOM_TILE), 1024)


@dataclass
class AtomOpResult:
    op: str
    instruction: str
    report: "ops.MemReport"
    ms: float
    gatoms: float  # 1e9 atomics per second
    gbs: float     # GB/s of operand bytes


@dataclass
class AtomTestResult:
    slots: int
    contributors: int
    per_op: dict = field(default_factory=dict)  # name -> AtomOpResult
    ticket: dict = field(default_factory=dict)  # (bits, C) -> MemReport
    chain: dict = field(default_factory=dict)   # name -> MemReport
    seconds: float = 0.0

    @property
    def reports(self):
        return ([r.report for r in self.per_op.values()]
                + list(self.ticket.values()) + list(self.chain.values()))

    @property
    def bad_dwords(self) -> int:
        return sum(r.bad_dwords for r in self.reports)

    @property
    def clean(self) -> bool:
        return self.bad_dwords == 0


def run_ticket(device, draws, counters, wide, report):
    """One ticket run into `report`: draw, then the two check kernels."""
    import torch

    dtype = torch.int64 if wide else torch.int32
    cnt = torch.zeros(counters, dtype=dtype, device=device)
    tickets = torch.full((draws,), -1, dtype=dtype, device=device)
    where = torch.full((-(-draws // ops.ATOM_TILE), 2), -1, dtype=torch.int32,
                       device=device)
    perm = torch.empty(counters * -(-draws // counters), dtype=torch.int32,
                       device=device)
    ops.atom_ticket(cnt, tickets, where)
    ops.atom_ticket_check(cnt, tickets, perm, report)
    return cnt, tickets, where


def run_chain(device, op, slots, seed, rounds):
    """`rounds` rounds of a chain op over fresh memory and the final compare;
    returns the MemReport."""
    import torch

    storage, buf = slot_buffer(op, slots, device)
    gold_storage, gold = slot_buffer(op, slots, device)
    report = ops.mem_report_new(device)
    where = torch.full((chain_wgs(slots), 2), -1, dtype=torch.int32,
                       device=device)
    ops.atom_fill(buf, op, seed)
    for r in range(rounds):
        ops.atom_chain_round(buf, op, seed, r, report, where)
    ops.atom_gold(gold, op, seed, rounds)
    ops.buf_compare(storage, gold_storage, report)
    return ops.mem_report_read(report)


def atomtest(device=None, op_names=None, slots=1 << 20, contributors=64,
             seed=0, rotate=True, returning=False, ticket_draws=1 << 20,
             ticket_counters=(1, 8, 64, 1024), chain_rounds=3):
    """Run every op (default: all reduce ops) once at `slots` x
    min(contributors, the op's cap): fill, gold, reduce, bitwise compare;
    then ticket mode for 32- and 64-bit counters and `chain_rounds` rounds
    of every chain op. Returns an AtomTestResult; nothing is judged by a
    rate."""
    import torch

    device = torch.device("cuda", torch.cuda.current_device()) \
        if device is None else torch.device(device)
    names = list(op_names) if op_names is not None else \
        list(ops.ATOM_REDUCE_OPS)
    result = AtomTestResult(slots=int(slots), contributors=int(contributors))
    t0 = time.perf_counter()
    with torch.cuda.device(device):
        for name in names:
            if name in ops.ATOM_CHAIN_OPS:
                continue
            W = min(int(contributors), w_cap(name))
            storage, buf = slot_buffer(name, slots, device)
            gold_storage, gold = slot_buffer(name, slots, device)
            report = ops.mem_report_new(device)
            ops.atom_fill(buf, name, seed)
            ops.atom_gold(gold, name, seed, W)
            ev0 = torch.cuda.Event(enable_timing=True)
            ev1 = torch.cuda.Event(enable_timing=True)
            ev0.record()
            if returning:
                ops.atom_reduce(buf, name, seed, W, rotate=rotate,
                                returning=True, gold=gold, report=report)
            else:
                ops.atom_reduce(buf, name, seed, W, rotate=rotate)
            ev1.record()
            ops.buf_compare(storage, gold_storage, report)
            rep = ops.mem_report_read(report)
            ms = ev0.elapsed_time(ev1)
            atoms = float(slots) * W
            result.per_op[name] = AtomOpResult(
                op=name, instruction=ops.ATOM_OPS[name][2], report=rep, ms=ms,
                gatoms=atoms / ms / 1e6 if ms > 0 else 0.0,
                gbs=atoms * slot_bytes(name) / ms / 1e6 if ms > 0 else 0.0)
        if ticket_draws:
            for wide in (False, True):
                for C in ticket_counters:
                    report = ops.mem_report_new(device)
                    run_ticket(device, int(ticket_draws), int(C), wide, report)
                    result.ticket[(64 if wide else 32, int(C))] = \
                        ops.mem_report_read(report)
        if chain_rounds:
            for name in ops.ATOM_CHAIN_OPS:
                if op_names is not None and name not in names:
                    continue
                result.chain[name] = run_chain(device, name, slots, seed,
                                               int(chain_rounds))
    result.seconds = time.perf_counter() - t0
    return result
