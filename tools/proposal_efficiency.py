#!/usr/bin/env python3
"""Statistical efficiency of the chemistry proposals: uniform2 against CauchySchwarz on the C2 cc-pVDZ walk (COUNTER discipline).

  python tools/proposal_efficiency.py [--targets 1e5 1e6] [--steps 20000] [--equil 2000] [--block 500] [--time-sym]

--time-sym walks the same molecule in the conventions of the shipped HCI decks (time_sym = t, z = 1, hf_symmetry = 1): the walkers are
representatives (up <= dn), and both proposals take the second pathway through the time-reversed determinant.

One JSON line per (proposal, w_abs_gen_target): ms_per_step of sqmc_gpu_run, the k_spawn time per step from the library's HIP
events (a separate pass of --timed-steps steps, sqmc_gpu_set_timing), E_proj with its error bar from --block-step blocks of the
timed run (ratio of the block sums of numerator and denominator), and err^2 x time (Ha^2 s for the --steps steps), the figure a
user picks a proposal by: the smaller, the less GPU time for a given error bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")


def measure(H, host, proposal, target, args):
    w = H.GpuWalk(host, target, rng_mode=H.RNG_COUNTER, proposal=proposal)
    try:
        w.run(args.equil, keep_stats=False)
        w.g.set_timing(2)
        spawn = []
        for _ in range(args.timed_steps):
            w.step()
            spawn.append(sum(ms for name, ms in w.g.timing() if "spawn" in name))
        w.g.set_timing(0)
        t0 = time.perf_counter()
        stats, _ = w.run(args.steps)
        dt = time.perf_counter() - t0
        st = np.asarray(stats).reshape(args.steps, -1)
        nb = args.steps // args.block
        num = st[:nb * args.block, 3].reshape(nb, args.block).sum(axis=1)
        den = st[:nb * args.block, 2].reshape(nb, args.block).sum(axis=1)
        e_blk = num / den
        e = float(num.sum() / den.sum())
        err = float(np.std(e_blk, ddof=1) / np.sqrt(nb))
        return {"proposal": {"uniform": "uniform2", "cauchyschwarz": "CauchySchwarz"}[proposal], "w_abs_gen_target": target,
                "time_sym": bool(host.time_sym), "z": int(host.z),
                "steps": args.steps, "ms_per_step": dt / args.steps * 1e3, "k_spawn_ms_per_step": float(np.median(spawn)),
                "e_proj": e, "e_proj_err": err, "blocks": nb, "block_steps": args.block,
                "err2_x_time_Ha2s": err * err * dt, "n_walkers": int(w.g.num_walkers())}
    finally:
        w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=float, nargs="+", default=[1e5, 1e6])
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--equil", type=int, default=2000)
    ap.add_argument("--timed-steps", type=int, default=100)
    ap.add_argument("--block", type=int, default=500)
    ap.add_argument("--time-sym", action="store_true", help="time_sym = t, z = 1, hf_symmetry = 1 (the c2_hci conventions)")
    args = ap.parse_args()
    import torch  # noqa: F401  one libamdhip64 per process
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    for target in args.targets:
        for proposal in ("uniform", "cauchyschwarz"):
            host = (H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1) if args.time_sym
                    else H.ChemHost(FCIDUMP, 8, 4, "d2h"))
            print(json.dumps(measure(H, host, proposal, target, args)), flush=True)


if __name__ == "__main__":
    main()
