#!/usr/bin/env python3
"""The distribution of the spawn-weight multiplier x = abs(weight_j)/tau = |H_ij| / p(i -> j) per proposal (uniform2 and
CauchySchwarz on C2 with 8 electrons, fast_heatbath on the 10-electron system), read from the walk's own histograms
(sqmc_gpu_set_spawn_diagnostics) after a fixed number of steps: max / min ratio, 1/max (the tau at which no spawn is heavier than
its parent's share), the share of proposals with x tau > 1, quantiles of x from the unit-wide bins (upper bin edges), and the
time of a step with the diagnostics on and off.  One JSON line per proposal, appended to --out as well.

--overhead measures what the diagnostic mode costs instead (profiles/spawn_hist_overhead.json, key "cost_when_on"): the uniform2 walk
at the bench size and at 10^6 walkers, two timed regions each of (a) the default pipelined step, (b) the same step un-pipelined
(SQMC_NO_PIPELINE=1, diagnostics off) and (c) the diagnostics on, which runs un-pipelined too.  (c) - (b) is the counting itself,
(b) - (a) the pipelining given up.  The file's other key, "off_must_be_free", is ten runs of
`python bench.py --gpus 1 --steps 2000 --warmup 200`, alternating between a checkout of the parent commit and this tree."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
CASES = [("uniform2", 8, 4, "uniform"), ("CauchySchwarz", 8, 4, "cauchyschwarz"), ("fast_heatbath", 10, 5, "heatbath")]
QUANTILES = (0.5, 0.9, 0.99, 0.999, 0.9999)


def timed_run(walk, torch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, totals = walk.run(steps, keep_stats=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, totals


def overhead(path, torch, H):
    """cost_when_on of profiles/spawn_hist_overhead.json; the other keys of the file are kept"""
    rows = []
    for target, steps in ((1e5, 2000), (1e6, 600)):
        hst = H.ChemHost(FCIDUMP, 8, 4, "d2h")
        walk = H.GpuWalk(hst, target, w_begin=1e4, seed=H.rank_seed((1346, 5634, 6635, 4361), 0))
        for _ in range(10):
            walk.run(500, keep_stats=False)
            if walk.pc.reached == 2:
                break
        else:
            raise RuntimeError("the walk did not reach its target population")
        walk.g.set_chained_runs(True)
        walk.run(200, keep_stats=False)
        off = [timed_run(walk, torch, steps)[0] for _ in range(2)]
        os.environ["SQMC_NO_PIPELINE"] = "1"             # read at every step
        walk.run(50, keep_stats=False)
        off_np = [timed_run(walk, torch, steps)[0] for _ in range(2)]
        del os.environ["SQMC_NO_PIPELINE"]
        walk.g.set_spawn_diagnostics(True)
        walk.run(50, keep_stats=False)
        walk.g.reset_spawn_diagnostics()
        on, totals = [], None
        for _ in range(2):
            ms, totals = timed_run(walk, torch, steps)
            on.append(ms)
        d = walk.spawn_diagnostics()
        walk.g.set_chained_runs(False)
        walk.close()
        m = lambda v: sum(v) / len(v)
        rows.append({"w_abs_gen_target": target, "steps": steps, "ms_per_step_off": off, "ms_per_step_off_unpipelined": off_np, "ms_per_step_on": on,
                     "children_per_step": float(totals[15]) / steps, "bins_occupied": int((d["bins"] > 0).sum()), "max_ratio": d["max_ratio"],
                     "min_ratio": d["min_ratio"], "ratio_on_over_off": m(on) / m(off), "ratio_on_over_off_unpipelined": m(on) / m(off_np),
                     "ms_pipelining_given_up": m(off_np) - m(off), "ms_counting": m(on) - m(off_np)})
        print(json.dumps(rows[-1]), flush=True)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["cost_when_on"] = rows
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--overhead", nargs="?", const=os.path.join(ROOT, "profiles", "spawn_hist_overhead.json"), default=None, metavar="JSON",
                    help="measure the cost of the diagnostic mode instead and write it into this file")
    ap.add_argument("--steps", type=int, default=2000, help="steps the histograms are accumulated over (and each timed region)")
    ap.add_argument("--equil", type=int, default=1000)
    ap.add_argument("--target", type=float, default=1e5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spawn_hist.jsonl"))
    a = ap.parse_args()
    import torch            # one libamdhip64 per process
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    if a.overhead:
        return overhead(a.overhead, torch, H)
    lines = []
    for name, nelec, nup, proposal in CASES:
        hst = H.ChemHost(FCIDUMP, nelec, nup, "d2h")
        kw = dict(mwalk=int(4 * (a.target / 0.5 + 1000) * 1.5)) if proposal == "heatbath" else {}
        walk = H.GpuWalk(hst, a.target, w_begin=min(a.target, 1e4), seed=H.rank_seed((1346, 5634, 6635, 4361), 0), proposal=proposal, **kw)
        walk.run(a.equil, keep_stats=False)
        walk.g.set_chained_runs(True)
        walk.run(200, keep_stats=False)
        ms_off, _ = timed_run(walk, torch, a.steps)
        walk.g.set_spawn_diagnostics(True)
        walk.run(50, keep_stats=False)
        walk.g.reset_spawn_diagnostics()
        ms_on, totals = timed_run(walk, torch, a.steps)
        d = walk.spawn_diagnostics()
        walk.g.set_chained_runs(False)
        tau = walk.setup.tau
        n = d["bins"].astype(np.float64)
        cum = np.cumsum(n) / n.sum()
        upper = np.arange(1, len(n) + 1)                 # bin b holds [b - 1, b)
        # x tau > 1  <=>  x > 1/tau: whole bins above the one that holds 1/tau (a lower bound on the share)
        first_above = int(np.floor(1.0 / tau)) + 1
        line = {"proposal": name, "system": "C2 cc-pVDZ r=1.24253, %d electrons" % nelec, "w_abs_gen_target": a.target, "steps": a.steps, "tau": tau,
                "proposals": int(n.sum()), "children_per_step": float(totals[15]) / a.steps,
                "max_ratio": d["max_ratio"], "max_ratio_level": d["max_ratio_level"], "min_ratio": d["min_ratio"], "tau_for_max_weight_1": 1.0 / d["max_ratio"],
                "tau_times_max_ratio": tau * d["max_ratio"], "share_x_tau_above_1": float(n[first_above:].sum() / n.sum()),
                "share_weightless_or_below_1": float(n[0] / n.sum()),
                "quantiles_of_x_upper_bin_edge": {str(q): int(upper[np.searchsorted(cum, q)]) for q in QUANTILES},
                "singles": int(d["bins_single"].sum()), "doubles": int(d["bins_double"].sum()), "last_bin": int(d["bins"][-1]), "n_nan": d["n_nan"],
                "ms_per_step_diagnostics_off": ms_off, "ms_per_step_diagnostics_on": ms_on}
        walk.close()
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
