#!/usr/bin/env python3
"""bench.py — flagship benchmark of the MI355X K3S enablement stack.

Measures the stack's headline metric (BASELINE.json): **HIP STREAM triad
GB/s** on 1..N MI355X GPUs — the GPU payload that our smoke pod runs where
the reference stack ran `nvidia-smi` (/root/reference/nvidia-smi.yaml:13;
the reference publishes no GB/s-class number, so vs_baseline is null and
the measured value becomes the recorded baseline).

One "step" = one STREAM triad sweep `a = b + s*c` over three fp32 buffers
of --buffer-mib MiB each (bytes moved per step = 3 x buffer bytes, STREAM
convention). Multi-GPU runs are launched by torch.distributed.run with one
rank per GPU; each rank owns its own buffers (weak scaling) and the
reported value is the whole-job aggregate GB/s computed with the MAX
elapsed time over ranks.

Contract (driver): rank 0 prints exactly one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--gpus", type=int, default=None,
                   help="number of GPUs (defaults to WORLD_SIZE or 1)")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--buffer-mib", type=int, default=1024,
                   help="MiB per buffer (3 buffers per GPU)")
    p.add_argument("--variant", choices=["auto", "plain", "nt"], default="auto",
                   help="plain or non-temporal loads/stores (auto measures both"
                        " during warmup and picks the faster globally)")
    p.add_argument("--graph", choices=["auto", "on", "off"], default="off",
                   help="capture the step in a hipGraph and replay it. "
                        "Measured on MI355X: the ~10-16us graph-replay floor "
                        "exceeds the ~3.5us eager launch for this 0.5ms "
                        "single-kernel step (6494 vs 6438 GB/s), so eager is "
                        "the default; the option remains for launch-bound "
                        "configurations (tiny buffers)")
    p.add_argument("--scalar", type=float, default=2.5)
    p.add_argument("--seed", type=int, default=0,
                   help="seed of the input buffers (rank r uses seed + r), so "
                        "two runs with the same arguments see the same data")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last step "
                        "computed to DIR/<name>.npy (float32): the triad's "
                        "output buffer `a`, or a fixed seeded sample of it "
                        "when it is larger than the dump budget")
    p.add_argument("--full", action="store_true",
                   help="also run the checks that the headline figure does "
                        "not need: at N>1 the RCCL transport self-diagnosis "
                        "(debug-log capture, per-transport channel counts in "
                        "config.rccl_transports)")
    return p.parse_args(argv)


# --dump-outputs budget: 64 MB over all ranks, of which we use a quarter
DUMP_MAX_ELEMS = (16 << 20) // 4


def sample_indices(n, max_elems, seed):
    """Fixed, seeded sample of positions in a length-n output: everything
    when it fits, else sorted random positions that always include both
    ends (same n, max_elems and seed -> same positions in every build)."""
    import torch
    if n <= max_elems:
        return None
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    idx = torch.randint(0, n, (max_elems,), generator=g, dtype=torch.int64)
    idx[0], idx[-1] = 0, n - 1
    return idx.sort().values


def dump_outputs(out_dir, a, *, rank, world_size, seed):
    """Write the timed path's output buffer as float32 .npy (one file per
    rank at N>1, the budget split evenly between ranks)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    idx = sample_indices(a.numel(), DUMP_MAX_ELEMS // world_size, seed)
    out = a if idx is None else a[idx.to(a.device)]
    name = "a" if world_size == 1 else f"a_rank{rank}"
    np.save(os.path.join(out_dir, name + ".npy"),
            out.detach().to("cpu", torch.float32).numpy())


# multi-GPU self-diagnosis lives in the package so the in-pod payloads
# (k3samd.parallel.allreduce) share the exact same logic
from k3samd.utils.rccl_diag import (  # noqa: E402
    assert_unique_device_binding, canonical_device_ids,
    enable_rccl_debug_capture, gather_transport_counts,
    parse_rccl_transports,
)


def build_result(*, value, n_gpus, steps, warmup, ms_per_step, buffer_mib,
                 variant):
    """Assemble the contract JSON (separated out for CPU-side tests)."""
    return {
        "metric": "hip_stream_triad_gbps",
        "value": round(value, 1),
        "unit": "GB/s",
        "n_gpus": n_gpus,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,  # reference publishes no bandwidth number
        "dtype": "fp32",
        "data": "synthetic",
        "config": {
            "model": "hip_stream_triad",
            "buffer_MiB": buffer_mib,
            "n_buffers": 3,
            "variant": variant,
            "parallelism": f"dp{n_gpus}",
        },
    }


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    # the aggregate is computed from ranks that actually ran: WORLD_SIZE is
    # the source of truth; --gpus is a cross-check only (never an inflator)
    n_gpus = world_size
    if args.gpus is not None and args.gpus != world_size:
        print(f"# note: --gpus {args.gpus} != WORLD_SIZE {world_size}; "
              f"reporting n_gpus={world_size}", file=sys.stderr)

    # CPU rehearsal of the exact torchrun path (gloo, no GPU): same
    # rendezvous, barriers, max-over-ranks reduction and JSON contract,
    # with a torch-eager triad standing in for the HIP kernel. The output
    # is stamped "rehearsal" so it can never pass as a measurement.
    rehearsal = os.environ.get("K3SAMD_BENCH_REHEARSAL") == "1"

    if not rehearsal and not torch.cuda.is_available():
        print("bench.py requires a GPU (run on the MI355X box; "
              "set K3SAMD_BENCH_REHEARSAL=1 for the CPU dry-run)",
              file=sys.stderr)
        return 1

    rccl_log = None
    dist = None
    if world_size > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        if args.full and not rehearsal:
            rccl_log = enable_rccl_debug_capture()
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        dist.init_process_group(backend="gloo" if rehearsal else "nccl",
                                rank=rank, world_size=world_size)

    if rehearsal:
        device = torch.device("cpu")
    else:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        if dist is not None:
            # fail loudly if two ranks share a physical GPU (halves the
            # aggregate silently otherwise)
            assert_unique_device_binding(dist, device, rank)

    if not rehearsal:
        from k3samd import ops
        if not ops.native_available():
            print("k3samd native extension missing — refusing to run a "
                  "fallback", file=sys.stderr)
            return 2

    buffer_mib = args.buffer_mib
    if rehearsal:
        buffer_mib = min(buffer_mib, 4)  # keep the dry-run light
    n = buffer_mib * (1 << 20) // 4  # fp32 elements per buffer
    torch.manual_seed(args.seed + rank)  # same arguments -> same inputs
    b = torch.rand(n, device=device)
    c = torch.rand(n, device=device)
    a = torch.empty_like(b)
    buffer_bytes = n * 4
    step_bytes = 3 * buffer_bytes

    def run_step(nt: bool):
        if rehearsal:
            torch.add(b, c, alpha=args.scalar, out=a)
        else:
            ops.stream_triad(a, b, c, args.scalar, nontemporal=nt)

    def sync():
        if not rehearsal:
            torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()

    # ---- variant selection (globally consistent across ranks) ----
    if args.variant == "auto" and not rehearsal:
        timings = []
        for nt in (False, True):
            for _ in range(5):
                run_step(nt)
            sync()
            t0 = time.perf_counter()
            for _ in range(10):
                run_step(nt)
            sync()
            timings.append(time.perf_counter() - t0)
        # nccl collectives need device tensors
        t = torch.tensor(timings, dtype=torch.float64, device=device)
        if dist is not None:
            dist.all_reduce(t)  # sum over ranks -> same decision everywhere
        use_nt = bool(t[1] < t[0])
    else:
        use_nt = args.variant == "nt"
    variant = "nt" if use_nt else "plain"

    # ---- optional hipGraph capture of one step ----
    graph = None
    if args.graph in ("auto", "on") and not rehearsal:
        try:
            g = torch.cuda.CUDAGraph()
            # side-stream warmup required before capture
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run_step(use_nt)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                run_step(use_nt)
            graph = g
        except Exception as e:  # pragma: no cover - device dependent
            if args.graph == "on":
                raise
            print(f"# graph capture unavailable, eager launches: {e}",
                  file=sys.stderr)

    def do_step():
        if graph is not None:
            graph.replay()
        else:
            run_step(use_nt)

    # ---- warmup ----
    for _ in range(args.warmup):
        do_step()
    sync()

    # ---- timed region ----
    barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        do_step()
    sync()
    elapsed = time.perf_counter() - t0
    barrier()

    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if dist is not None:
        # keep every rank's own time too: a straggler shows up as one
        # low per-rank rate, not just a depressed aggregate
        all_t = [torch.zeros_like(t) for _ in range(world_size)]
        dist.all_gather(all_t, t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    t_max = float(t[0])

    value = n_gpus * step_bytes * args.steps / t_max / 1e9
    ms_per_step = t_max / args.steps * 1e3
    if dist is not None and rank == 0:
        per_rank = [round(step_bytes * args.steps / float(x[0]) / 1e9, 1)
                    for x in all_t]
        print(f"# per-rank GB/s: {per_rank} (straggler = lowest)",
              file=sys.stderr)

    # ---- RCCL transport self-diagnosis (N>1 on the GPU path) ----
    transports = None
    if dist is not None and rccl_log is not None:
        transports = gather_transport_counts(dist, rccl_log, rank, world_size)
        if rank == 0:
            print(f"# rccl transports: {transports or 'no log captured'}",
                  file=sys.stderr)
            non_p2p = sum(v for k, v in transports.items() if k != "P2P")
            if transports and (transports.get("P2P", 0) == 0 or non_p2p):
                print("# WARNING: RCCL channels not all xGMI P2P — check "
                      "device injection / IPC mode", file=sys.stderr)

    if args.dump_outputs:
        sync()
        dump_outputs(args.dump_outputs, a, rank=rank, world_size=world_size,
                     seed=args.seed)

    if rank == 0:
        res = build_result(value=value, n_gpus=n_gpus, steps=args.steps,
                           warmup=args.warmup, ms_per_step=ms_per_step,
                           buffer_mib=buffer_mib, variant=variant)
        res["config"]["hip_graph"] = graph is not None
        if rehearsal:
            res["rehearsal"] = True  # gloo/CPU dry-run, NOT a measurement
        if transports is not None:
            res["config"]["rccl_transports"] = transports
        print(json.dumps(res))

    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
