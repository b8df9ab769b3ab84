#!/usr/bin/env python3
"""Time of a sharded fast_heatbath step: the shipped C2 cc-pVDZ integrals with 10 electrons (the system bench.py --proposal heatbath
times on one GPU), N ranks, determinants sharded by hash ownership, two walker slots per child.

  python tools/heatbath_sharded_time.py --ranks N --steps K [--warmup W] [--path inlib|gloo]

The launcher starts one child per rank the way bench.py does (it never touches the GPU) and forwards rank 0's one JSON line:
{"ms_per_step", "world", "path", ...}.  path inlib: the library's own exchange (RCCL, the pipelined sqmc_gpu_shard_run); gloo: the
caller-driven three phases (sqmc_gpu_shard_begin / _pack / _finish) with the exchanges through torch.distributed.  The walk runs
--equil untimed steps to its target population first.  bench.py --gpus N keeps timing the uniform sharded walk; this tool is the
heat-bath counterpart."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")


def launch(args):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out = procs[0].stdout.read()
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out.decode())
    return max(abs(c) for c in rcs)


def rank_main(args):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    json_fd = os.dup(1)
    os.dup2(2, 1)                                   # stdout carries the JSON line only
    local = rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # caller-driven exchange, or the carrier of the RCCL unique id
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(local)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    w = H.ShardedWalk(hst, args.target * world, rank, world, proposal=args.proposal)
    if args.path == "inlib":
        w.attach_rccl()

    def steps(n, keep=False):
        rows = None
        if args.path == "inlib":
            rows, _ = w.run(n, keep_stats=keep)
        else:
            rows = np.array([w.step() for _ in range(n)])
        torch.cuda.synchronize()
        dist.barrier()
        return rows

    steps(args.equil + args.warmup)
    t0 = time.perf_counter()
    rows = steps(args.steps, keep=True)
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    line = {"ms_per_step": 1e3 * float(t[0]) / args.steps, "world": world, "path": args.path, "proposal": args.proposal, "steps": args.steps,
            "target_per_rank": args.target, "mwalk": int(w.g.mwalk), "w_abs_gen": float(w.w_abs),
            "nwalk_global_mean": float(rows[:, 5].mean()), "children_per_step_rank0": float(rows[:, 15].mean()),
            "energy": float((rows[:, 3] * np.sign(rows[:, 2])).sum() / np.abs(rows[:, 2]).sum()),
            "workload": "C2 cc-pVDZ integrals with 10 electrons (10e,26o, D2h; synthetic) semistochastic walk, sharded by hash ownership"}
    if rank == 0:
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    w.close()
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--equil", type=int, default=2000)
    ap.add_argument("--target", type=float, default=1e5, help="w_abs_gen target per rank")
    ap.add_argument("--path", default="inlib", choices=["inlib", "gloo"])
    ap.add_argument("--proposal", default="heatbath", choices=["heatbath", "uniform"], help="uniform: the same system and sizes with the uniform proposal, for comparison")
    args = ap.parse_args()
    if "RANK" not in os.environ:
        return launch(args)
    return rank_main(args)


if __name__ == "__main__":
    sys.exit(main())
