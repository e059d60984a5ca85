"""CDNA4 HIP kernel bindings.

The native extension (``k3samd/_C*.so``) is compiled in-tree for gfx950 by
``k3samd.build``. On a GPU machine a missing extension is a hard error —
there is deliberately no silent eager/PyTorch fallback for the compute path
(the kernels ARE the product, the MI355X analog of the reference's in-pod
``nvidia-smi`` payload, /root/reference/nvidia-smi.yaml:13).
"""

from __future__ import annotations

from dataclasses import dataclass, field

_C = None
_import_error: Exception | None = None

try:
    import torch  # noqa: F401  — the extension links against torch's libs
    from k3samd import _C  # type: ignore[attr-defined]
except ImportError as e:  # extension not built (CPU-only dev box is fine)
    _import_error = e


def _require_native():
    if _C is None:
        raise RuntimeError(
            "k3samd native extension is not built. Run "
            "`python -m k3samd.build` (or __graft_entry__.build()). "
            f"Original import error: {_import_error}"
        )
    return _C


def native_available() -> bool:
    return _C is not None


def stream_triad(a, b, c, s, nontemporal=False):
    """a = b + s*c over fp32 tensors, 16B/lane vectorized CDNA4 kernel."""
    _require_native().stream_triad(a, b, c, float(s), nontemporal)


def stream_copy(a, b, nontemporal=False):
    _require_native().stream_copy(a, b, nontemporal)


def stream_scale(a, c, s, nontemporal=False):
    _require_native().stream_scale(a, c, float(s), nontemporal)


def stream_add(a, b, c, nontemporal=False):
    _require_native().stream_add(a, b, c, nontemporal)


def mfma_throughput(out, iters, shape=16):
    """Issue `iters` MFMA groups per wave (shape 16 = v_mfma_f32_16x16x32,
    shape 32 = v_mfma_f32_32x32x16); returns FLOPs issued."""
    return _require_native().mfma_throughput(out, int(iters), int(shape))


# Validated on MI355X silicon (first gpurun, 2026-09-13): layout 0 — lane l
# holds A[l&15][(l>>4)*8 + j] (k-contiguous 8-element groups) — matches the
# hardware fragment mapping of v_mfma_f32_16x16x32_bf16 (max err 1.9e-6 vs
# torch fp32 matmul); layout 1 does not.
MFMA_LAYOUT = 0


def mfma_gemm16(A, B, layout=MFMA_LAYOUT):
    """Single-tile D[16,16] = A[16,32] @ B[32,16] via one bf16 MFMA."""
    return _require_native().mfma_gemm16(A, B, int(layout))


def mx_gemm16(A, B, fmt=0):
    """Single-tile D[16,16] = dequant(A[16,128]) @ dequant(B[128,16]) via
    one block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales.

    fmt 0 = fp8 e4m3 (A uint8 [16,128]; B uint8 [16,128] packed
    column-major: row c = column c of B). fmt 4 = fp4 e2m1 (packed two
    elements per byte, low nibble = even k: A [16,64], B [16,64]).
    """
    return _require_native().mx_gemm16(A, B, int(fmt))


# ---- HBM pattern memory test (kernels in hip/memtest_kernels.h) ----

MEM_PATTERN_ADDR = 0
MEM_PATTERN_WALK = 1
MEM_PATTERN_CHECKER = 2

MEM_LOG_SLOTS = 16
MEM_REPORT_LEN = 8 + 3 * MEM_LOG_SLOTS

_U64 = (1 << 64) - 1


def _spec4(pattern, seed, invert, cell_offset):
    """The (pattern, seed, invert, cell_offset) arguments as the native
    layer takes them: seed and offset wrapped to 64 bits."""
    return int(pattern), int(seed) & _U64, bool(invert), int(cell_offset) & _U64


@dataclass
class MemReport:
    """Host-side view of the device report tensor."""

    bad_dwords: int
    bad_bits: int
    first_bad_dword: int | None  # global dword index g = 4*cell + k
    xor_or: int
    log: list = field(default_factory=list)  # <= 16 (g, expected, actual)

    @property
    def clean(self) -> bool:
        return self.bad_dwords == 0


def mem_report_new(device):
    """Fresh report tensor: int64[56], all zero except first_bad_dword = -1
    (all-ones, the identity of the unsigned min)."""
    import torch

    _require_native()
    r = torch.zeros(MEM_REPORT_LEN, dtype=torch.int64)
    r[2] = -1
    return r.to(device)


def mem_fill(buf, pattern, seed, invert=False, cell_offset=0,
             nontemporal=True):
    """Store the pattern over `buf` (any contiguous GPU tensor whose byte
    size is a multiple of 16)."""
    _require_native().mem_fill(buf, *_spec4(pattern, seed, invert, cell_offset),
                               bool(nontemporal))


def mem_verify(buf, report, pattern, seed, invert=False, cell_offset=0):
    """Compare `buf` with the pattern and accumulate into `report`.
    No host sync: read the report once with mem_report_read()."""
    _require_native().mem_verify(buf, report,
                                 *_spec4(pattern, seed, invert, cell_offset))


def mem_verify_fill(buf, report, old, new, cell_offset=0, nontemporal=True):
    """March element: verify pattern `old` and overwrite with `new` in one
    pass. `old` and `new` are (pattern, seed, invert) triples."""
    op, os_, oi = old
    np_, ns, ni = new
    _require_native().mem_verify_fill(
        buf, report, int(op), int(os_) & _U64, bool(oi), int(np_),
        int(ns) & _U64, bool(ni), int(cell_offset) & _U64, bool(nontemporal))


# ---- verified bf16 MFMA GEMM (kernels in hip/gemm_kernels.h) ----

GEMM_TILE_M = 128
GEMM_TILE_N = 128
GEMM_TILE_K = 64
GEMM_EXACT_MAX_K = 32768  # 256 * K <= 2^23: every partial sum exact in fp32


def gemm_fill(buf, which, seed, rows, cols):
    """Write generator operands into the stored [rows, cols] matrix `buf`
    in its own dtype (bfloat16, float16, int8, float32 or float64; cols a
    whole number of 16-byte cells): which = 0 is A[M,K]; which = 1 is
    Bt[N,K], whose element [n][k] is gemm_operand(seed, 1, row=k, col=n)."""
    _require_native().gemm_fill(buf, int(which), int(seed) & _U64, int(rows),
                                int(cols))


def gemm_bf16_nt(A, Bt, out=None, where=None):
    """C[M,N] (fp32) = A[M,K] @ Bt[N,K].T with v_mfma_f32_16x16x32_bf16,
    for any bf16 data. M % 128 == N % 128 == K % 64 == 0. `where`
    (int32 [tiles, 2]) receives each 128x128 tile's XCC_ID and HW_ID."""
    return _require_native().gemm_bf16_nt(A, Bt, out, where)


def gemm_ref_int(A, Bt, out=None):
    """The same product by int32 VALU arithmetic (no MFMA), as fp32. For
    operands holding integers in [-128, 127], K <= 32768."""
    return _require_native().gemm_ref_int(A, Bt, out)


# ---- verified fp16 / int8 / fp32 / fp64 GEMM (hip/gemm_dense_kernels.h) ----


def _gemm_formats():
    try:
        import torch
    except ImportError:
        return {}
    return {"bf16": (torch.bfloat16, torch.float32, 64),
            "fp16": (torch.float16, torch.float32, 64),
            "int8": (torch.int8, torch.int32, 128),
            "fp32": (torch.float32, torch.float32, 32),
            "fp64": (torch.float64, torch.float64, 16)}


# name -> (operand dtype, result dtype, K-step in elements): one K-step is
# 128 bytes of every operand row. bf16 is gemm_bf16_nt / gemm_ref_int; the
# other four are gemm_dense_nt / gemm_dense_ref_int.
GEMM_FORMATS = _gemm_formats()


def gemm_dense_nt(A, Bt, out=None, where=None):
    """C[M,N] = A[M,K] @ Bt[N,K].T on the matrix pipe of A's dtype, for any
    data: float16 (v_mfma_f32_16x16x32_f16, C float32), int8
    (v_mfma_i32_16x16x64_i8, C int32), float32 (v_mfma_f32_16x16x4_f32, C
    float32) or float64 (v_mfma_f64_16x16x4_f64, C float64). M % 128 ==
    N % 128 == 0, K a whole number of the format's K-steps (GEMM_FORMATS).
    `where` as for gemm_bf16_nt."""
    return _require_native().gemm_dense_nt(A, Bt, out, where)


def gemm_dense_ref_int(A, Bt, out=None):
    """The same product by int32 VALU arithmetic (no MFMA), in the format's
    result dtype. For operands holding integers in [-128, 127], K <= 32768;
    a float32 result is exact only while |sum| <= 2^24."""
    return _require_native().gemm_dense_ref_int(A, Bt, out)


def buf_compare(buf, expected, report):
    """Bitwise compare of two equally sized GPU buffers, accumulated into
    a mem_report_new() report; dword indices count 32-bit elements (two
    per float64 element, low half first)."""
    _require_native().buf_compare(buf, expected, report)


# ---- verified MX (fp8 / fp4 block-scaled) GEMM (hip/mx_gemm_kernels.h) ----

MX_FMT_FP8 = 0  # e4m3 (OCP e4m3fn), one byte per element
MX_FMT_FP4 = 4  # e2m1, two elements per byte, low nibble = even k
MX_EXACT_MAX_K = 8192  # 1024 * K <= 2^23: every partial sum exact in fp32


def mx_gemm16_scaled(A, SA, B, SB, fmt):
    """Single-tile D[16,16] = (A∘SA)[16,128] @ (B∘SB)[128,16] via one
    v_mfma_scale_f32_16x16x128_f8f6f4 with per-lane scale operands. A and B
    are packed as for mx_gemm16; SA and SB are uint8 [16,4], the E8M0 scale
    of (row of A or column of B, block of 32 k)."""
    return _require_native().mx_gemm16_scaled(A, SA, B, SB, int(fmt))


def mx_fill(elems, scales, which, seed, rows, k, fmt):
    """Write generator elements into the stored [rows, k] uint8 matrix
    `elems` (k bytes per row for fp8, k/2 for fp4) and its E8M0 scales into
    `scales` [rows, k/32]: which = 0 is A and SA; which = 1 is Bt and SB,
    with Bt[n][k] = operand(seed, 1, row=k, col=n)."""
    _require_native().mx_fill(elems, scales, int(which), int(seed) & _U64,
                              int(rows), int(k), int(fmt))


def mx_gemm_nt(A, SA, Bt, SB, fmt, out=None, where=None):
    """C[M,N] (fp32) = (A∘SA) @ (Bt∘SB).T with the block-scaled 16x16x128
    MFMA. M % 128 == N % 128 == 0; K % 128 == 0 (fp8) or K % 256 == 0
    (fp4). `where` as for gemm_bf16_nt."""
    return _require_native().mx_gemm_nt(A, SA, Bt, SB, int(fmt), out, where)


def mx_gemm_ref_int(A, SA, Bt, SB, fmt, out=None):
    """The same product by int32 VALU arithmetic (no MFMA), as fp32. For
    integer-valued fp8 elements or any fp4 codes, scales 127..129,
    K <= 8192."""
    return _require_native().mx_gemm_ref_int(A, SA, Bt, SB, int(fmt), out)


# ---- per-CU self-test (kernels in hip/cu_test_kernels.h) ----

CU_LDS_BYTES = 163840  # the whole LDS of one CU: one workgroup per CU
CU_LDS_CELLS = CU_LDS_BYTES // 16
CU_WG_THREADS = 256
CU_WAVES = 4
CU_FOLD_CELL_BIT = 1 << 40  # report cell index of the signature's LDS fold


def _inject_tensor(inject, cols):
    """None or a sequence of `cols`-tuples -> None or a CPU int64[n, cols]
    tensor (an empty list is None)."""
    if inject is None:
        return None
    import torch

    rows = [[int(v) for v in row] for row in inject]
    if not rows:
        return None
    if any(len(row) != cols for row in rows):
        raise ValueError(f"every inject row must have {cols} entries")
    return torch.tensor(rows, dtype=torch.int64)


def cu_lds_march(report, where, seed, passes=1, stop_after=4, inject=None,
                 dump=None):
    """March the whole 160 KiB LDS of every CU that runs a workgroup of the
    launch: `where` (int32 [wgs, 2]) sets the grid and receives each
    workgroup's XCC_ID and HW_ID; miscompares accumulate into `report`
    (dword g: workgroup g // 40960, LDS byte 4 * (g % 40960)). The last
    pass ends after phase `stop_after` (0..4); `dump` (int32 [wgs, 40960])
    receives the final LDS content. `inject` is a list of (wg, lds_dword,
    xor_mask, phase 0..3) planted in pass 0 after that phase's write."""
    _require_native().cu_lds_march(report, where, int(seed) & _U64,
                                   int(passes), int(stop_after),
                                   _inject_tensor(inject, 4), dump)


def cu_valu_signature(report, where, seed, rounds, expected, sig_out=None,
                      inject=None):
    """Run the VALU signature on every wave of the launch and compare with
    `expected` (int32 [64, 4] on the GPU, from cu_signature_expected()).
    `where` (int32 [4 * wgs, 2]) sets the grid and receives each wave's
    XCC_ID and HW_ID; report cell c = (wg * 4 + wave) * 64 + lane, dword k
    = datapath (cell CU_FOLD_CELL_BIT | c holds the cross-wave LDS fold).
    `sig_out` (int32 [256 * wgs, 4]) receives the compared cells; `inject`
    is a list of (wg, wave, lane, k 0..4, xor_mask)."""
    _require_native().cu_valu_signature(report, where, int(seed) & _U64,
                                        int(rounds), expected, sig_out,
                                        _inject_tensor(inject, 5))


def cu_signature_expected(seed, rounds):
    """The signature of one wave from the host code of hip/cu_pattern.h: a
    CPU int32 [64, 4] tensor of bit patterns. Needs no GPU."""
    return _require_native().cu_signature_expected(int(seed) & _U64,
                                                   int(rounds))


# ---- host-link (PCIe) test (kernels in hip/hostlink_kernels.h) ----
# Host buffers are pinned CPU tensors (tensor.pin_memory()); the kernels run
# on the current device and stream. `wgs` workgroups of 256 lanes walk the
# region, so bytes in flight on the link are 256 * 16 * 4 * wgs.

LINK_DEFAULT_WGS = 256  # per direction; link_duplex defaults to twice that
LINK_MAX_WGS = 4096
LINK_SLOT_BYTES = 64
LINK_CHASE_MAX_N = 1 << 26
LINK_CHASE_MAX_HOPS = 1 << 22


def link_pull_verify(host_buf, report, pattern, seed, invert=False,
                     cell_offset=0, wgs=LINK_DEFAULT_WGS):
    """The device reads pinned host memory and compares it with the pattern,
    accumulating into `report` (a GPU mem_report_new() tensor). No host
    sync."""
    _require_native().link_pull_verify(
        host_buf, report, *_spec4(pattern, seed, invert, cell_offset), int(wgs))


def link_push_fill(host_buf, pattern, seed, invert=False, cell_offset=0,
                   wgs=LINK_DEFAULT_WGS):
    """The device stores the pattern into pinned host memory. No host sync:
    synchronise before the host reads the buffer."""
    _require_native().link_push_fill(
        host_buf, *_spec4(pattern, seed, invert, cell_offset), int(wgs))


def _link_spec(spec):
    """(pattern, seed, invert[, cell_offset]) -> four checked ints."""
    pattern, seed, invert, *rest = spec
    if len(rest) > 1:
        raise ValueError("a link spec is (pattern, seed, invert[, cell_offset])")
    return _spec4(pattern, seed, invert, rest[0] if rest else 0)


def link_duplex(pull_buf, report, pull_spec, push_buf, push_spec,
                wgs=2 * LINK_DEFAULT_WGS):
    """One launch of `wgs` >= 2 workgroups: the even ones pull-verify
    `pull_buf` into `report`, the odd ones push-fill `push_buf`, so both
    directions of the link are loaded at once. The specs are (pattern, seed,
    invert[, cell_offset]); the two regions must not overlap."""
    _require_native().link_duplex(pull_buf, report, *_link_spec(pull_spec),
                                  push_buf, *_link_spec(push_spec), int(wgs))


def link_chase(host_buf, n, hops, out):
    """One lane makes `hops` dependent loads through the `n`-slot chase table
    in pinned `host_buf` (from link_chase_fill). `out` (GPU int64[4])
    receives the final index, the XOR of the visited indices, the elapsed
    wall_clock64 ticks and `hops`."""
    _require_native().link_chase(host_buf, int(n), int(hops), out)


def link_wall_clock_khz(device=0):
    """wall_clock64 ticks per millisecond of GPU `device` (an index)."""
    return _require_native().link_wall_clock_khz(int(device))


def link_host_fill(buf, pattern, seed, invert=False, cell_offset=0,
                   threads=0):
    """Write the pattern into a CPU tensor with up to 16 host threads
    (0 = chosen from the size). Needs no GPU."""
    _require_native().link_host_fill(
        buf, *_spec4(pattern, seed, invert, cell_offset), int(threads))


def link_host_verify(buf, pattern, seed, invert=False, cell_offset=0,
                     threads=0) -> MemReport:
    """Compare a CPU tensor with the pattern on the host. The result does
    not depend on `threads`; the log holds the 16 lowest bad dwords. Needs
    no GPU."""
    return _mem_report_decode(_require_native().link_host_verify(
        buf, *_spec4(pattern, seed, invert, cell_offset),
        int(threads)).tolist())


def link_chase_fill(buf, n, seed):
    """Write the `n`-slot chase table (64 bytes per slot, dword 0 = next
    index) into a CPU tensor of 64 * n bytes. Needs no GPU."""
    _require_native().link_chase_fill(buf, int(n), int(seed) & _U64)


def link_chase_expected(n, seed, hops):
    """(final, xor) of `hops` hops from slot 0 of a clean table, from the
    host code of hip/hostlink_pattern.h. Needs no GPU."""
    return tuple(_require_native().link_chase_expected(
        int(n), int(seed) & _U64, int(hops)))


# ---- global-atomics integrity test (kernels in hip/atom_kernels.h) ----
# A slot is one 4- or 8-byte element of `buf`; W contributors (workgroups)
# each apply one operand of hip/atom_pattern.h to every slot. Report dword
# indices count 32-bit words of the buffer (two per 8-byte slot, low first).

ATOM_MAX_CONTRIBUTORS = 4096
ATOM_MAX_PACKED = 240
ATOM_TILE = 256  # slots per tile = lanes per workgroup
ATOM_CHAIN_OPS = ("swap", "swap64", "cas", "cas64")


def _atom_ops():
    try:
        import torch
    except ImportError:
        return {}
    i32, i64 = torch.int32, torch.int64
    table = {}
    for name in ("add", "and", "or", "xor", "smin", "smax", "umin", "umax"):
        table[name] = (i32, 4, "global_atomic_" + name, ATOM_MAX_CONTRIBUTORS)
    for name in ("add", "and", "or", "xor", "smin", "smax", "umin", "umax"):
        table[name + "64"] = (i64, 8, f"global_atomic_{name}_x2",
                              ATOM_MAX_CONTRIBUTORS)
    table["addf32"] = (torch.float32, 4, "global_atomic_add_f32",
                       ATOM_MAX_CONTRIBUTORS)
    table["addf64"] = (torch.float64, 8, "global_atomic_add_f64",
                       ATOM_MAX_CONTRIBUTORS)
    table["minf64"] = (torch.float64, 8, "global_atomic_min_f64",
                       ATOM_MAX_CONTRIBUTORS)
    table["maxf64"] = (torch.float64, 8, "global_atomic_max_f64",
                       ATOM_MAX_CONTRIBUTORS)
    table["pkaddbf16"] = (i32, 4, "global_atomic_pk_add_bf16", ATOM_MAX_PACKED)
    table["pkaddf16"] = (i32, 4, "global_atomic_pk_add_f16", ATOM_MAX_PACKED)
    table["swap"] = (i32, 4, "global_atomic_swap", ATOM_MAX_CONTRIBUTORS)
    table["swap64"] = (i64, 8, "global_atomic_swap_x2", ATOM_MAX_CONTRIBUTORS)
    table["cas"] = (i32, 4, "global_atomic_cmpswap", ATOM_MAX_CONTRIBUTORS)
    table["cas64"] = (i64, 8, "global_atomic_cmpswap_x2",
                      ATOM_MAX_CONTRIBUTORS)
    return table


# name -> (tensor dtype of a slot buffer, slot bytes, the instruction the op
# compiles to, W cap). The order is the native op id; the last four are the
# chain ops (their "W" is the round count). A packed slot is two 16-bit
# floats in an int32.
ATOM_OPS = _atom_ops()
ATOM_REDUCE_OPS = tuple(n for n in ATOM_OPS if n not in ATOM_CHAIN_OPS)


def atom_op_id(op) -> int:
    """Native id of an op given by name (or already by id)."""
    if isinstance(op, str):
        try:
            return list(ATOM_OPS).index(op)
        except ValueError:
            raise ValueError(f"unknown atomics op {op!r}") from None
    return int(op)


def atom_fill(buf, op, seed):
    """Store atom_init(op, seed, slot) into every slot of `buf` with plain
    stores."""
    _require_native().atom_fill(buf, atom_op_id(op), int(seed) & _U64)


def atom_gold(buf, op, seed, W):
    """Store atom_expected(op, seed, slot, W) into every slot: one thread
    per slot folds the operands in registers, no atomic is issued."""
    _require_native().atom_gold(buf, atom_op_id(op), int(seed) & _U64, int(W))


def atom_reduce(buf, op, seed, W, rotate=False, returning=False, gold=None,
                report=None, drop=None):
    """W workgroups each apply their operand to every slot of `buf` with
    the op's atomic instruction. `rotate` starts workgroup w at tile
    (40503 * w) % tiles; `drop` = (w, tile) makes that workgroup skip that
    tile. `returning` uses the value-returning form and checks each returned
    value against the final value in `gold` (order-independent invariants),
    accumulating violations into `report`."""
    dw, dt = (-1, -1) if drop is None else (int(drop[0]), int(drop[1]))
    _require_native().atom_reduce(buf, atom_op_id(op), int(seed) & _U64, int(W),
                                  bool(rotate), bool(returning), gold, report,
                                  dw, dt)


def atom_ticket(counters, tickets, where):
    """Draw i of len(tickets) takes a ticket from counter i % len(counters)
    with a returning fetch-add and stores it in tickets[i]. `counters` (int32
    or int64, zeroed by the caller) and `tickets` share a dtype; `where`
    (int32 [ceil(draws / 256), 2]) receives each workgroup's placement."""
    _require_native().atom_ticket(counters, tickets, where)


def atom_ticket_check(counters, tickets, perm, report):
    """Prove without atomics that each counter's tickets are a permutation
    of 0..n-1 and that it ended at n. `perm` (int32 [C * ceil(draws / C)])
    is scratch. Report dword c * ceil(draws / C) + t is (counter c, ticket
    t): expected t; dword C * ceil(draws / C) + c is counter c's final
    value."""
    _require_native().atom_ticket_check(counters, tickets, perm, report)


def atom_chain_round(buf, op, seed, round, report, where):
    """Round `round` of swap / swap64 / cas / cas64: every slot moves from
    v_round to v_round+1 with one returning atomic (cas: after one that must
    fail) and the returned value is checked into `report`. `where` (int32
    [wgs, 2]) sets the grid; tile t is served by workgroup (t + round) %
    wgs."""
    _require_native().atom_chain_round(buf, atom_op_id(op), int(seed) & _U64,
                                       int(round), report, where)


def atom_init(op, seed, slot) -> int:
    """Bits a slot holds before any atomic, from the host code of
    hip/atom_pattern.h. Needs no GPU."""
    return _require_native().atom_init(atom_op_id(op), int(seed) & _U64,
                                       int(slot) & _U64)


def atom_operand(op, seed, slot, w, W) -> int:
    """Bits contributor `w` of `W` applies to a slot. Needs no GPU."""
    return _require_native().atom_operand(atom_op_id(op), int(seed) & _U64,
                                          int(slot) & _U64, int(w), int(W))


def atom_expected(op, seed, slot, W) -> int:
    """Bits of the slot after all W contributors. Needs no GPU."""
    return _require_native().atom_expected(atom_op_id(op), int(seed) & _U64,
                                           int(slot) & _U64, int(W))


def atom_shape_ok(op, slots, W) -> bool:
    """The caps every entry point applies: 1 <= slots <= 2^30 and 1 <= W <=
    the op's cap."""
    return _require_native().atom_shape_ok(atom_op_id(op), int(slots), int(W))


def mem_report_read(report) -> MemReport:
    """Copy the report to the host (this is the synchronisation point)."""
    return _mem_report_decode(report.cpu().tolist())


def _mem_report_decode(values) -> MemReport:
    r = [int(v) for v in values]
    n_log = min(max(r[4], 0), MEM_LOG_SLOTS)
    log = [(r[8 + 3 * i] & _U64, r[9 + 3 * i] & 0xFFFFFFFF,
            r[10 + 3 * i] & 0xFFFFFFFF) for i in range(n_log)]
    first = r[2] & _U64
    return MemReport(bad_dwords=r[0], bad_bits=r[1],
                     first_bad_dword=None if first == _U64 else first,
                     xor_or=r[3] & 0xFFFFFFFF, log=log)
