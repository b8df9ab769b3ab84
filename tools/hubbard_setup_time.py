#!/usr/bin/env python3
"""Wall time of HubbardHost.setup_walk (real-space Hubbard, 'hubbard2') on one GPU: the kept host construction (_setup_walk_host:
Python loops for the first-order space, one hamiltonian_batch call per Psi_T determinant for C(T)) against the device path (one
connection-generator call per level and one for C(T)).  Cases: 4x4 periodic (8,8) and 6x6 periodic (4,4), n_levels 2 and 3, U/t = 4.
Per case one warm-up of each path, then --reps repetitions that alternate the two in one process, a device synchronise before each
clock read; median and min-max of each path and the sizes of the spaces.  Prints one JSON line per case and writes them as the
"cases" entry of profiles/hubbard_setup.json (--out: another file)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((4, 4, 8, 8), 2), ((4, 4, 8, 8), 3), ((6, 6, 4, 4), 2), ((6, 6, 4, 4), 3)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubbard_setup.json"), help="the file whose \"cases\" entry the lines replace")
    ap.add_argument("--max-levels", type=int, default=3, help="skip cases with more levels than this")
    a = ap.parse_args()
    import torch            # one libamdhip64 per process
    import numpy as np
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    kw = dict(n_truncate_trial_wf=20, size_deterministic=500, tau_multiplier=0.5)
    lines = []
    for (lx, ly, nup, ndn), n_levels in CASES:
        if n_levels > a.max_levels:
            continue
        hst = H.HubbardHost(lx, ly, True, nup, ndn, 1.0, 4.0)
        g = hst.gpu()
        try:
            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = fn(g, n_levels=n_levels, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, s
            paths = (("host", hst._setup_walk_host), ("device", hst.setup_walk))
            last = {name: timed(fn)[1] for name, fn in paths}                  # one warm-up each
            t = {name: [] for name, _ in paths}
            for _ in range(a.reps):
                for name, fn in paths:
                    dt, last[name] = timed(fn)
                    t[name].append(dt)
            space = hst.first_order_space(n_levels, g)
        finally:
            g.close()
        same = all(np.array_equal(getattr(last["host"], k), getattr(last["device"], k)) for k in ("psi_up", "psi_dn", "psi_c", "imp_up", "imp_dn", "ct_up", "ct_dn", "ct_num", "ct_den"))
        line = {"metric": "setup_walk wall time", "unit": "s", "lattice": "%dx%d periodic" % (lx, ly), "nup": nup, "ndn": ndn, "n_levels": n_levels, "reps": a.reps,
                "first_order_space": int(len(space[0])), "psi_t": int(len(last["device"].psi_up)), "deterministic": int(len(last["device"].imp_up)),
                "c_t": int(len(last["device"].ct_up)), "paths_agree_bit_for_bit": bool(same)}
        for name in t:
            line[name] = {"median": statistics.median(t[name]), "min": min(t[name]), "max": max(t[name]), "all": t[name]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    doc = {}
    if os.path.exists(a.out):                      # the file's other entries (the benchmark lines recorded beside the cases) stay
        with open(a.out) as f:
            doc = json.load(f)
    doc["cases"] = lines
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
