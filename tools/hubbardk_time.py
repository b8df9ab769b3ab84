#!/usr/bin/env python3
"""Time of a semistochastic walk step with the plane-wave Hubbard operator (hubbardk) on one GPU: 8x8, 7 up and 7 down
electrons, U/t = 4, w_abs_gen_target 1e5, the steps inside sqmc_gpu_run as bench.py times them.  Prints one JSON line.
(7 + 7 is the largest filling of 64 orbitals whose determinant space, C(64,7)^2 = 3.9e17, fits the library's 63-bit sort keys;
13 + 13 would need 88 bits and is refused by the context.)
Without the options below the run and its JSON line are what they always were.
--space-sym Z P: the same walk among the representatives of the z / p symmetry sector (needs nup = ndn and a start determinant of
momentum 0: --nup 5 --ndn 5 is a closed shell); adds "space_sym".  --repeat N: N timed runs of --steps steps instead of one, the
ms_per_step of each in "repeats" (the line's own value and ms_per_step are the last run's).  --stages: 20 more steps at the end under the
stage timers (sqmc_gpu_set_timing), "spawn_share" = the share of the stages whose name holds 'spawn' (k_spawn) in their total."""
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
    ap.add_argument("--space-sym", type=int, nargs=2, metavar=("Z", "P"), default=None, help="walk in the symmetry-adapted basis of the sector z, p (default: off)")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--stages", action="store_true", help="report k_spawn's share of a step from the stage timers")
    a = ap.parse_args()
    import torch            # one libamdhip64 per process
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    lx, ly = (int(v) for v in a.lattice.lower().split("x"))
    sym = dict(space_sym=True, z=a.space_sym[0], p=a.space_sym[1]) if a.space_sym else {}
    hst = H.HubbardKHost(lx, ly, a.nup, a.ndn, 1.0, 4.0, **sym)
    walk = H.GpuWalk(hst, a.target, w_begin=min(a.target, 1e4), n_truncate_trial_wf=20, size_deterministic=500, tau_multiplier=a.tau_multiplier, mwalk=int(8 * (a.target / 0.5 + 500)),
                     seed=H.rank_seed((1346, 5634, 6635, 4361), 0))
    walk.run(a.equil, keep_stats=False)
    walk.g.set_chained_runs(True)
    walk.run(a.warmup, keep_stats=False)
    repeats = []
    for _ in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats, totals = walk.run(a.steps, keep_stats=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        repeats.append(dt / a.steps * 1e3)
    walk.g.set_chained_runs(False)
    extra = {}
    if a.repeat > 1:
        extra["repeats"] = repeats
    if a.space_sym:
        extra["space_sym"] = a.space_sym
    if a.stages:
        walk.g.set_timing(2)
        stage = {}
        for _ in range(20):
            walk.step()
            for name, ms in walk.g.timing():
                stage[name] = stage.get(name, 0.0) + ms
        walk.g.set_timing(0)
        extra["spawn_share"] = sum(v for k, v in stage.items() if "spawn" in k) / max(sum(stage.values()), 1e-30)
    e = float((stats[:, 3]).sum() / stats[:, 2].sum())
    print(json.dumps({"metric": "walker-steps/sec", "value": float(totals[5]) / dt, "unit": "walker-steps/s", "ms_per_step": dt / a.steps * 1e3,
                      "steps": a.steps, "warmup": a.warmup, **extra,
                      "config": {"workload": "%dx%d Hubbard U/t=4, %d up %d dn, plane waves (hubbardk), semistochastic walk, w_abs_gen_target=%g, "
                                             "size_deterministic=500, Psi_T 20 dets, tau_multiplier %g" % (lx, ly, a.nup, a.ndn, a.target, a.tau_multiplier),
                                 "n_imp": int(len(walk.setup.imp_up)), "tau": walk.setup.tau, "occupied_dets_per_step": float(totals[5]) / a.steps,
                                 "spawns_per_step": float(totals[15]) / a.steps, "projected_energy": e}}))
    walk.close()


if __name__ == "__main__":
    main()
