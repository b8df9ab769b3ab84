#!/usr/bin/env python3
"""Time of a semistochastic walk step with the plane-wave Hubbard operator (hubbardk) on one GPU: 8x8, 7 up and 7 down
electrons, U/t = 4, w_abs_gen_target 1e5, the steps inside sqmc_gpu_run as bench.py times them.  Prints one JSON line.
(7 + 7 is the largest filling of 64 orbitals whose determinant space, C(64,7)^2 = 3.9e17, fits the library's 63-bit sort keys;
13 + 13 would need 88 bits and is refused by the context.)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--equil", type=int, default=2000)
    ap.add_argument("--target", type=float, default=1e5)
    ap.add_argument("--lattice", default="8x8")
    ap.add_argument("--nup", type=int, default=7)
    ap.add_argument("--ndn", type=int, default=7)
    ap.add_argument("--tau-multiplier", type=float, default=0.1, help="tau = this / the spectral range bound.  A determinant has nup ndn (nsites - nup) = 2793 "
                    "connections of |H| = U / nsites here: at 0.5 the spawned weight per step is about the parents' own and the population overshoots MWALK "
                    "before population control has acted")
    a = ap.parse_args()
    import torch            # one libamdhip64 per process
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    lx, ly = (int(v) for v in a.lattice.lower().split("x"))
    hst = H.HubbardKHost(lx, ly, a.nup, a.ndn, 1.0, 4.0)
    walk = H.GpuWalk(hst, a.target, w_begin=min(a.target, 1e4), n_truncate_trial_wf=20, size_deterministic=500, tau_multiplier=a.tau_multiplier, mwalk=int(8 * (a.target / 0.5 + 500)),
                     seed=H.rank_seed((1346, 5634, 6635, 4361), 0))
    walk.run(a.equil, keep_stats=False)
    walk.g.set_chained_runs(True)
    walk.run(a.warmup, keep_stats=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats, totals = walk.run(a.steps, keep_stats=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    walk.g.set_chained_runs(False)
    e = float((stats[:, 3]).sum() / stats[:, 2].sum())
    print(json.dumps({"metric": "walker-steps/sec", "value": float(totals[5]) / dt, "unit": "walker-steps/s", "ms_per_step": dt / a.steps * 1e3,
                      "steps": a.steps, "warmup": a.warmup,
                      "config": {"workload": "%dx%d Hubbard U/t=4, %d up %d dn, plane waves (hubbardk), semistochastic walk, w_abs_gen_target=%g, "
                                             "size_deterministic=500, Psi_T 20 dets, tau_multiplier %g" % (lx, ly, a.nup, a.ndn, a.target, a.tau_multiplier),
                                 "n_imp": int(len(walk.setup.imp_up)), "tau": walk.setup.tau, "occupied_dets_per_step": float(totals[5]) / a.steps,
                                 "spawns_per_step": float(totals[15]) / a.steps, "projected_energy": e}}))
    walk.close()


if __name__ == "__main__":
    main()
