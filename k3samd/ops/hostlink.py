"""Host-link (PCIe) integrity and bandwidth test: numpy reference of the
pointer chase and the phase driver.

``reference_chase_table`` / ``reference_chase`` are an independent
re-implementation of ``hip/hostlink_pattern.h`` in numpy integer arithmetic;
the data pattern's reference stays ``k3samd.ops.memtest.reference_pattern``.

``hostlink`` moves verified data across the link in every way a workload
does: kernels that read and write pinned host memory (pull, push, both at
once), the copy engines (H2D, D2H, both at once) and a dependent-load chase
for the round-trip latency. It covers the path between host DRAM and this
GPU only; the host buffers are not NUMA-bound, and GPU-to-GPU links are a
different test (``mi-allreduce``).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from k3samd import ops
from k3samd.ops import MemReport
from k3samd.ops.memtest import ADDR, CHECKER, WALK

PHASES = ("pull", "push", "duplex", "h2d", "d2h", "sdma_duplex")

_CHASE_MUL = 0x9E3779B1
_U64 = (1 << 64) - 1


def _check_chase_n(n):
    n = int(n)
    if n < 2 or n > ops.LINK_CHASE_MAX_N or n & (n - 1):
        raise ValueError("chase n must be a power of two in 2 .. 2^26")
    return n


def reference_chase_table(n, seed):
    """The chase table as uint32[n, 16]: dword 0 of slot i is next(i), the
    rest of the 64-byte slot is zero."""
    n = _check_chase_n(n)
    inc = np.uint64((int(seed) & 0xFFFFFFFF) | 1)
    i = np.arange(n, dtype=np.uint64)
    # n <= 2^26 keeps 0x9E3779B1 * i below 2^58: no wrap-around involved
    nxt = (np.uint64(_CHASE_MUL) * i + inc) & np.uint64(n - 1)
    table = np.zeros((n, ops.LINK_SLOT_BYTES // 4), dtype=np.uint32)
    table[:, 0] = nxt.astype(np.uint32)
    return table


def reference_chase(n, seed, hops):
    """(final, xor) of `hops` dependent loads from slot 0: the last loaded
    index and the XOR of every loaded index."""
    nxt = reference_chase_table(n, seed)[:, 0].tolist()
    i = x = 0
    for _ in range(int(hops)):
        i = nxt[i]
        x ^= i
    return i, x


@dataclass
class LinkPhase:
    """One phase over all passes: what was found and how fast it moved."""

    report: MemReport
    gbps: float  # bytes over the event-timed transfers; duplex: both ways
    bytes_moved: int
    ms: float


@dataclass
class ChaseResult:
    n: int
    hops: int
    final: int
    xor: int
    expected_final: int
    expected_xor: int
    ticks: int
    ns_per_hop: float

    @property
    def ok(self) -> bool:
        return (self.final, self.xor) == (self.expected_final,
                                          self.expected_xor)


@dataclass
class HostlinkResult:
    pull: LinkPhase
    push: LinkPhase
    duplex: LinkPhase
    h2d: LinkPhase
    d2h: LinkPhase
    sdma_duplex: LinkPhase
    chase: ChaseResult

    @property
    def phases(self) -> dict:
        return {name: getattr(self, name) for name in PHASES}

    @property
    def bad_dwords(self) -> int:
        return sum(p.report.bad_dwords for p in self.phases.values())

    @property
    def bad_bits(self) -> int:
        return sum(p.report.bad_bits for p in self.phases.values())

    @property
    def first_bad_phase(self):
        for name, p in self.phases.items():
            if not p.report.clean:
                return name
        return None if self.chase.ok else "chase"

    @property
    def clean(self) -> bool:
        return self.first_bad_phase is None


def _merge(a: MemReport, b: MemReport) -> MemReport:
    firsts = [r.first_bad_dword for r in (a, b) if r.first_bad_dword is not None]
    return MemReport(bad_dwords=a.bad_dwords + b.bad_dwords,
                     bad_bits=a.bad_bits + b.bad_bits,
                     first_bad_dword=min(firsts) if firsts else None,
                     xor_or=a.xor_or | b.xor_or,
                     log=(a.log + b.log)[:ops.MEM_LOG_SLOTS])


def _march(s):
    """The memtest march as four specs: address-unique, its complement,
    walking one, checkerboard."""
    return [(ADDR, s, False), (ADDR, s, True), (WALK, s, False),
            (CHECKER, s, False)]


def inject_flips(host_buf, n_flips):
    """XOR one bit into `n_flips` dwords of a CPU tensor, spread from the
    first dword to the last; returns [(dword, mask)]."""
    words = host_buf.numpy().view(np.uint32)
    flips = []
    for f in range(int(n_flips)):
        g = f * (len(words) - 1) // max(int(n_flips) - 1, 1)
        mask = 1 << (f % 32)
        words[g] ^= np.uint32(mask)
        flips.append((g, mask))
    return flips


def hostlink(mib=64, passes=1, seed=0, device=None, inject=None, wgs=None,
             chase_n=1 << 16, chase_hops=10000):
    """Run every phase over `mib` MiB per direction and return a
    HostlinkResult.

    Per pass p and phase index k the seed is seed + 7 * p + k, and each
    phase marches ADDR -> ~ADDR -> WALK -> CHECKER, so data left by an
    earlier step or phase cannot satisfy a later one. The second region of
    a duplex phase uses seed + 1 and cell indices that follow the first
    region's. Verifies that are not themselves the transfer run outside
    the timed interval. `inject` plants that many single-bit flips into the
    host buffer before the first pull, to rehearse the detector.
    """
    import torch

    dev = (torch.device("cuda", torch.cuda.current_device())
           if device is None else torch.device(device))
    nbytes = int(mib) << 20
    if nbytes <= 0 or int(passes) < 1:
        raise ValueError("mib and passes must be >= 1")
    n_cells = nbytes // 16
    wgs = ops.LINK_DEFAULT_WGS if wgs is None else int(wgs)
    chase_n = _check_chase_n(chase_n)

    with torch.cuda.device(dev):
        host_r = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        host_w = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        dev_in = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dev_out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        side = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        dev_reports = {k: ops.mem_report_new(dev) for k in PHASES}
        host_reports = {k: MemReport(0, 0, None, 0) for k in PHASES}
        ms = dict.fromkeys(PHASES, 0.0)
        moved = dict.fromkeys(PHASES, 0)

        def timed(name, n_bytes, fn):
            ev0.record()
            fn()
            ev1.record()
            ev1.synchronize()
            ms[name] += ev0.elapsed_time(ev1)
            moved[name] += n_bytes

        def host_check(name, spec, cell_offset=0):
            host_reports[name] = _merge(
                host_reports[name],
                ops.link_host_verify(host_w, *spec, cell_offset=cell_offset))

        def both_copies():
            cur = torch.cuda.current_stream()
            done = []
            for stream, dst, src in ((side[0], dev_in, host_r),
                                     (side[1], host_w, dev_out)):
                stream.wait_stream(cur)
                with torch.cuda.stream(stream):
                    dst.copy_(src, non_blocking=True)
                done.append(stream)
            for stream in done:
                cur.wait_stream(stream)

        for p in range(int(passes)):
            base = int(seed) + 7 * p
            for spec in _march(base & _U64):
                ops.link_host_fill(host_r, *spec)
                if inject and p == 0 and spec == (ADDR, base & _U64, False):
                    inject_flips(host_r, inject)
                timed("pull", nbytes, lambda: ops.link_pull_verify(
                    host_r, dev_reports["pull"], *spec, wgs=wgs))
            for spec in _march((base + 1) & _U64):
                timed("push", nbytes,
                      lambda: ops.link_push_fill(host_w, *spec, wgs=wgs))
                host_check("push", spec)
            for spec in _march((base + 2) & _U64):
                other = (spec[0], (spec[1] + 1) & _U64, spec[2])
                ops.link_host_fill(host_r, *spec)
                timed("duplex", 2 * nbytes, lambda: ops.link_duplex(
                    host_r, dev_reports["duplex"], spec, host_w,
                    other + (n_cells,), wgs=max(2, min(2 * wgs,
                                                       ops.LINK_MAX_WGS))))
                host_check("duplex", other, n_cells)
            for spec in _march((base + 3) & _U64):
                ops.link_host_fill(host_r, *spec)
                timed("h2d", nbytes,
                      lambda: dev_in.copy_(host_r, non_blocking=True))
                ops.mem_verify(dev_in, dev_reports["h2d"], *spec)
            for spec in _march((base + 4) & _U64):
                ops.mem_fill(dev_out, *spec)
                timed("d2h", nbytes,
                      lambda: host_w.copy_(dev_out, non_blocking=True))
                host_check("d2h", spec)
            for spec in _march((base + 5) & _U64):
                other = (spec[0], (spec[1] + 1) & _U64, spec[2])
                ops.link_host_fill(host_r, *spec)
                ops.mem_fill(dev_out, *other, cell_offset=n_cells)
                timed("sdma_duplex", 2 * nbytes, both_copies)
                ops.mem_verify(dev_in, dev_reports["sdma_duplex"], *spec)
                host_check("sdma_duplex", other, n_cells)

        chase_seed = (int(seed) + 6) & _U64
        table = torch.empty(ops.LINK_SLOT_BYTES * chase_n, dtype=torch.uint8,
                            pin_memory=True)
        ops.link_chase_fill(table, chase_n, chase_seed)
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        ops.link_chase(table, chase_n, chase_hops, out)
        final, xor, ticks, hops = (int(v) for v in out.cpu().tolist())
        want = ops.link_chase_expected(chase_n, chase_seed, chase_hops)
        khz = ops.link_wall_clock_khz(dev.index or 0)
        chase = ChaseResult(n=chase_n, hops=hops, final=final, xor=xor,
                            expected_final=want[0], expected_xor=want[1],
                            ticks=ticks, ns_per_hop=ticks * 1e6 / khz / hops)

        phases = {}
        for name in PHASES:
            report = _merge(ops.mem_report_read(dev_reports[name]),
                            host_reports[name])
            phases[name] = LinkPhase(
                report=report, bytes_moved=moved[name], ms=ms[name],
                gbps=moved[name] / (ms[name] * 1e6) if ms[name] > 0 else 0.0)
    return HostlinkResult(chase=chase, **phases)
