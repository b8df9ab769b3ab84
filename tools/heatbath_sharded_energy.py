#!/usr/bin/env python3
"""The energy bound of tests/test_gpu_heatbath_sharded.py: the spread over seeds of the single-GPU fast_heatbath walk's
outs[10:, 3].sum() / outs[10:, 2].sum() at the sizes the test uses (10 electrons, 40 steps, w_begin 2000, w_target 20000).

  python tools/heatbath_sharded_energy.py [--seeds N] > profiles/heatbath_sharded.json

Prints one JSON document: {"energy": {"single_gpu_seeds": [[seed, value], ...], "mean", "spread" (sample standard deviation),
"bound" (4 * spread), ...}}.  The two-rank sharded walk draws from other random streams than the single-GPU walk (every rank has
its own seed), so its energy is another sample of the same distribution; the test allows it four times the spread."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
NSTEPS, W_BEGIN, W_TARGET, SEED = 40, 2000, 20000, (1346, 5634, 6635, 4361)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    rows = []
    for k in range(args.seeds):
        seed = H.rank_seed(SEED, k)                  # k = 0: the seed of the tests' single-GPU walk
        w = H.GpuWalk(hst, W_TARGET, w_begin=W_BEGIN, seed=seed, mwalk=400000, proposal="heatbath")
        outs = np.array([w.step().copy() for _ in range(NSTEPS)])
        w.close()
        rows.append([list(seed), float(outs[10:, 3].sum() / outs[10:, 2].sum())])
    e = np.array([r[1] for r in rows])
    spread = float(e.std(ddof=1))
    doc = {"energy": {"quantity": "outs[10:, 3].sum() / outs[10:, 2].sum() of 40 steps, w_begin 2000, w_target 20000, C2 integrals with 10 electrons, fast_heatbath",
                      "single_gpu_seeds": rows, "mean": float(e.mean()), "spread": spread, "spread_is": "sample standard deviation over the seeds",
                      "bound": 4.0 * spread}}
    print(json.dumps(doc, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
