"""Per-CU self-test: the independent oracle of the VALU signature, the
decode of the placement registers, and the coverage-driven driver.

``reference_signature`` re-derives ``hip/cu_pattern.h`` without sharing
its arithmetic:

* the hash in masked uint64 numpy arithmetic;
* fp32 fma as ``float32(float64(f) * float64(a) + float64(b))``. This is
  exact: f and a have 24 significant bits each, so the product has at most
  48 with its last bit at 2^-47 or above (f >= 1 has lsb >= 2^-23, a >= 0.5
  has lsb 2^-24); b is a multiple of 2^-23 and the sum is below 16, so the
  float64 expression spans at most 2^3 .. 2^-47 = 51 bits, is computed
  without rounding, and the conversion to float32 rounds once — which is
  the definition of fmaf;
* fp64 fma with ``fractions.Fraction``: the exact rational f*a + b,
  converted by ``float()``, whose int/int division rounds correctly once;
* integers as masked Python / uint64 arithmetic, signed bytes by explicit
  sign extension.

``decode_hw_id`` / ``cu_key`` / ``coverage`` turn the ``{XCC_ID, HW_ID}``
pairs the kernels record (and the raw ``hw_id 0x...`` words that
``mi-stream --gemmtest`` and ``mi-mxgemm`` print) into a physical location.
``cutest`` launches both kernels over 4 x CU-count workgroups — each
declares the whole 160 KiB of LDS, so one is resident per CU — and
relaunches until every CU and every SIMD has been seen.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from k3samd import ops

_M32 = np.uint64(0xFFFFFFFF)
LANES = 64
LDS_DWORDS = ops.CU_LDS_BYTES // 4

SALT_F0, SALT_D0, SALT_U0 = 0xF32A0001, 0xF64A0002, 0x1A7E0003
SALT_FA, SALT_FB = 0xF32A0011, 0xF32A0012
SALT_DA, SALT_DB = 0xF64A0021, 0xF64A0022
SALT_UM, SALT_UC, SALT_UQ = 0x1A7E0031, 0x1A7E0032, 0x1A7E0033

# HW_ID fields: name -> (low bit, width), gfx9-family layout
HW_ID_FIELDS = {
    "wave": (0, 4), "simd": (4, 2), "pipe": (6, 2), "cu": (8, 4),
    "sh": (12, 1), "se": (13, 3), "tg": (16, 4), "vm": (20, 4),
    "queue": (24, 3), "state": (27, 3), "me": (30, 2),
}


def _mul32(a, b):
    return (a * np.uint64(b)) & _M32


def _hash(seed, r, salt):
    """lowbias32 over (lane 0..63, r, seed, salt) as a uint64[64] array
    masked to 32 bits after every multiply."""
    seed = int(seed) & ((1 << 64) - 1)
    lane = np.arange(LANES, dtype=np.uint64)
    h = _mul32(lane, 0x9E3779B1) ^ np.uint64((int(r) * 0x85EBCA6B) & 0xFFFFFFFF)
    h = h ^ np.uint64(seed & 0xFFFFFFFF)
    h = h ^ np.uint64(((seed >> 32) * 0xC2B2AE35) & 0xFFFFFFFF)
    h = h ^ np.uint64(salt)
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> np.uint64(15))
    h = _mul32(h, 0x846CA68B)
    return h ^ (h >> np.uint64(16))


def _sbytes(v):
    """The four bytes of each 32-bit value as signed Python ints."""
    v = int(v)
    out = []
    for i in range(4):
        b = (v >> (8 * i)) & 0xFF
        out.append(b - 256 if b >= 128 else b)
    return out


def _rotl1(v):
    return ((v << 1) | (v >> 31)) & 0xFFFFFFFF


def signature_chains(seed, rounds, perturb=None):
    """Generator over the oracle's state: yields (f, d, u) after the start
    values and after every round — f a float32[64] array, d a list of 64
    Python floats, u a list of 64 ints. `perturb` = (lane, xor_mask) changes
    one lane's starting u."""
    f = (1.0 + (_hash(seed, 0, SALT_F0) >> np.uint64(9)).astype(np.float64)
         * 2.0 ** -23).astype(np.float32)
    d = [1.0 + int(h) * 2.0 ** -32 for h in _hash(seed, 0, SALT_D0)]
    u = [int(h) for h in _hash(seed, 0, SALT_U0)]
    if perturb is not None:
        u[perturb[0]] ^= perturb[1] & 0xFFFFFFFF
    yield f, d, u
    for r in range(int(rounds)):
        a = 0.5 + (_hash(seed, r, SALT_FA) >> np.uint64(10)).astype(
            np.float64) * 2.0 ** -24
        b = 1.0 + (_hash(seed, r, SALT_FB) >> np.uint64(9)).astype(
            np.float64) * 2.0 ** -23
        f = (f.astype(np.float64) * a + b).astype(np.float32)
        da = [0.5 + int(h) * 2.0 ** -34 for h in _hash(seed, r, SALT_DA)]
        db = [1.0 + int(h) * 2.0 ** -32 for h in _hash(seed, r, SALT_DB)]
        d = [float(Fraction(x) * Fraction(y) + Fraction(z))
             for x, y, z in zip(d, da, db)]
        um = _hash(seed, r, SALT_UM)
        uc = _hash(seed, r, SALT_UC)
        uq = _hash(seed, r, SALT_UQ)
        stepped = []
        for lane in range(LANES):
            t = (u[lane] * (int(um[lane]) | 1) + int(uc[lane])) \
                & ((1 << 64) - 1)
            v = (t & 0xFFFFFFFF) ^ (t >> 32)
            dot = sum(x * y for x, y in zip(_sbytes(v), _sbytes(uq[lane])))
            stepped.append((v + dot) & 0xFFFFFFFF)
        dist = 1 << (r % 6)
        u = [stepped[lane] ^ _rotl1(stepped[lane ^ dist])
             for lane in range(LANES)]
        yield f, d, u


def reference_signature(seed, rounds, perturb=None):
    """The signature of one wave as uint32[64, 4]: d0 = fp32 chain bits,
    d1/d2 = low/high word of the fp64 chain, d3 = integer chain."""
    for f, d, u in signature_chains(seed, rounds, perturb):
        pass
    out = np.empty((LANES, 4), dtype=np.uint32)
    out[:, 0] = f.view(np.uint32)
    dbits = np.array(d, dtype=np.float64).view(np.uint64)
    out[:, 1] = (dbits & _M32).astype(np.uint32)
    out[:, 2] = (dbits >> np.uint64(32)).astype(np.uint32)
    out[:, 3] = np.array(u, dtype=np.uint64).astype(np.uint32)
    return out


def reference_fold(d3):
    """The signature kernel's fifth checked value from a lane's d3."""
    d3 = int(d3)
    out = 0
    for w in range(4):
        out ^= ((d3 << (w + 1)) | (d3 >> (31 - w))) & 0xFFFFFFFF
    return out


# ---- placement ----

def decode_hw_id(hw_id):
    """Every field of an HW_ID word (also the raw `hw_id 0x...` the GEMM
    payloads print) as a dict of ints."""
    hw_id = int(hw_id) & 0xFFFFFFFF
    return {name: (hw_id >> lo) & ((1 << width) - 1)
            for name, (lo, width) in HW_ID_FIELDS.items()}


def cu_key(xcc_id, hw_id):
    """One value per physical CU: XCC_ID[3:0] joined with the SE, SH and CU
    fields of HW_ID and nothing else."""
    return ((int(xcc_id) & 0xF) << 8) | ((int(hw_id) >> 8) & 0xFF)


def describe_key(key):
    return {"xcc": (key >> 8) & 0xF, "se": (key >> 5) & 7,
            "sh": (key >> 4) & 1, "cu": key & 0xF}


@dataclass
class Coverage:
    keys: set = field(default_factory=set)        # distinct CU keys
    simds: set = field(default_factory=set)       # distinct (key, SIMD)
    per_key: dict = field(default_factory=dict)   # key -> rows seen

    def update(self, other):
        self.keys |= other.keys
        self.simds |= other.simds
        for k, n in other.per_key.items():
            self.per_key[k] = self.per_key.get(k, 0) + n


def coverage(where):
    """Coverage of a recorded [rows, 2] table of {XCC_ID, HW_ID}."""
    cov = Coverage()
    for xcc, hw in np.asarray(where).reshape(-1, 2).tolist():
        key = cu_key(xcc, hw)
        cov.keys.add(key)
        cov.simds.add((key, decode_hw_id(hw)["simd"]))
        cov.per_key[key] = cov.per_key.get(key, 0) + 1
    return cov


def locate(g, kind):
    """Decode a report dword index. kind "lds": workgroup, LDS byte offset,
    cell and dword. kind "valu": workgroup, wave, lane and datapath k
    (0 fp32, 1/2 fp64 low/high, 3 integer, 4 the cross-wave LDS fold)."""
    g = int(g)
    if kind == "lds":
        wg, d = divmod(g, LDS_DWORDS)
        return {"wg": wg, "byte": 4 * d, "cell": d // 4, "k": d % 4}
    if kind == "valu":
        fold = bool((g >> 2) & ops.CU_FOLD_CELL_BIT)
        c = (g >> 2) & (ops.CU_FOLD_CELL_BIT - 1)
        return {"wg": c // 256, "wave": (c // 64) % 4, "lane": c % 64,
                "k": 4 if fold else g % 4}
    raise ValueError('kind must be "lds" or "valu"')


def _placed(loc, where_row):
    xcc, hw = int(where_row[0]), int(where_row[1])
    return {**loc, **describe_key(cu_key(xcc, hw)),
            "simd": decode_hw_id(hw)["simd"]}


def cutest(device="cuda:0", seed=0, passes=4, rounds=1024, max_launches=8):
    """Run both self-tests over the whole device; returns a dict.

    Each launch is 4 x multi_processor_count workgroups of either kernel.
    Launches repeat until the LDS kernel has been seen on every CU and the
    signature kernel on every SIMD of every CU, or `max_launches` is
    reached. Keys: lds / valu (MemReport), cus_total, cus_covered,
    simds_covered, launches, covered, lds_coverage / valu_coverage
    (Coverage) and miscompares (decoded location of every logged one; the
    LDS kernel records its workgroup's first wave only, so LDS entries
    carry no "simd").
    """
    import torch

    dev = torch.device(device)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    wgs = 4 * cus
    lds_report = ops.mem_report_new(dev)
    valu_report = ops.mem_report_new(dev)
    expected = ops.cu_signature_expected(seed, rounds).to(dev)
    lds_cov, valu_cov = Coverage(), Coverage()
    miscompares, seen = [], {"lds": 0, "valu": 0}
    launches = 0
    while launches < int(max_launches):
        lds_where = torch.full((wgs, 2), -1, dtype=torch.int32, device=dev)
        valu_where = torch.full((4 * wgs, 2), -1, dtype=torch.int32,
                                device=dev)
        ops.cu_lds_march(lds_report, lds_where, seed, passes)
        ops.cu_valu_signature(valu_report, valu_where, seed, rounds, expected)
        launches += 1
        lw, vw = lds_where.cpu().numpy(), valu_where.cpu().numpy()
        lds_cov.update(coverage(lw))
        valu_cov.update(coverage(vw))
        # decode new log records against THIS launch's placement
        for kind, report, table in (("lds", lds_report, lw),
                                    ("valu", valu_report, vw)):
            log = ops.mem_report_read(report).log
            for g, want, got in log[seen[kind]:]:
                loc = locate(g, kind)
                row = loc["wg"] if kind == "lds" \
                    else 4 * loc["wg"] + loc["wave"]
                placed = _placed(loc, table[row])
                if kind == "lds":
                    del placed["simd"]
                miscompares.append({"kind": kind, "g": g, "expected": want,
                                    "actual": got, **placed})
            seen[kind] = len(log)
        if len(lds_cov.keys) >= cus and len(valu_cov.simds) >= 4 * cus:
            break
    return {
        "lds": ops.mem_report_read(lds_report),
        "valu": ops.mem_report_read(valu_report),
        "cus_total": cus,
        "cus_covered": len(lds_cov.keys),
        "simds_covered": len(valu_cov.simds),
        "launches": launches,
        "covered": (len(lds_cov.keys) == cus
                    and len(valu_cov.simds) == 4 * cus),
        "lds_coverage": lds_cov,
        "valu_coverage": valu_cov,
        "miscompares": miscompares,
    }
