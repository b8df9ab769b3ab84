#!/usr/bin/env python3
"""Macro-iterations of orbital optimisation on the C2 fixture at one eps_var, beside the same number of natural-orbital turns.
Writes one JSON document (default profiles/orbopt_loop.json).

  optimised orbitals   HCI -> 1-RDM, 2-RDM -> host.optimize_orbitals_step -> ChemHost.with_integrals -> HCI -> ...
  natural orbitals     HCI -> 1-RDM -> host.natural_orbitals -> GpuChem.rotate_integrals -> ChemHost.with_integrals -> HCI -> ...

Per iteration: E_var, the number of determinants, and for the optimised orbitals max|g|, the step's scale and the fixed-coefficient
energies before and after it.  State 1 of a one-state run; nothing is promised about either loop, the record is what was measured.

--solver newton adds a third loop, "newton_orbitals": the same macro-iterations with host.optimize_orbitals_step(solver="newton"), the
Newton-CG step on the device's Hessian-vector products, with its products, stop reason and predicted change per iteration (write it
beside the other record: --out profiles/orbhess_loop.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--eps-var", type=float, default=2e-3)
ap.add_argument("--solver", choices=("diagonal", "newton"), default="diagonal")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbopt_loop.json"))
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)


def variational(host):
    g = host.gpu()
    try:
        g.set_hb_tables(*host.hb_tables(g))
        t0 = time.perf_counter()
        up, dn, w, e, _ = H.hci_variational(host, g, args.eps_var)
        return up, dn, np.asarray(w, float).reshape(len(up), -1)[:, 0], float(np.atleast_1d(e)[0]), time.perf_counter() - t0
    finally:
        g.close()


def loop(kind):
    host, rows = H.ChemHost(FCIDUMP, 8, 4, "d2h", hf_symmetry=1), []
    for it in range(args.iters + 1):
        up, dn, w, e, secs = variational(host)
        row = {"iteration": it, "e_var": e, "ndets": int(len(up)), "variational_stage_wall_s": secs}
        t0 = time.perf_counter()
        if kind in ("optimised", "newton"):
            r = H.optimize_orbitals_step(host, up, dn, w, solver="newton") if kind == "newton" else H.optimize_orbitals_step(host, up, dn, w)
            row.update({"max_gradient": r["max_gradient"], "gradient_norm": r["gradient_norm"], "max_kappa": r["max_kappa"], "scale": r["scale"],
                        "fixed_coefficient_energy_before": r["energy_before"], "fixed_coefficient_energy_after": r["energy_after"]})
            if kind == "newton":
                row.update({"hessian_vector_products": r["cg_iterations"], "cg_stop": r["cg_stop"], "predicted_change": r["predicted_change"]})
            packed = r["integrals"]
        else:
            D = H.hci_one_rdm(host, up, dn, w)
            G = H.spin_free_two_rdm(H.hci_two_rdm(host, up, dn, w))
            g = host.gpu()
            try:
                row["max_gradient"] = float(np.max(np.abs(g.orbital_gradient(D, G, "gradient")["gradient"])))
                packed = g.rotate_integrals(H.natural_orbitals(D, host.orbsym[1:host.norb + 1])[1])
            finally:
                g.close()
        row["step_wall_s"] = time.perf_counter() - t0
        rows.append(row)
        print(kind, json.dumps(row), flush=True)
        host = host.with_integrals(packed)
    return rows


doc = {"tool": "tools/orbopt_loop.py", "command": "python tools/orbopt_loop.py --iters %d --eps-var %g%s" % (args.iters, args.eps_var, " --solver newton" if args.solver == "newton" else ""),
       "system": "C2_r1.24253 cc-pVDZ, 8 electrons in 26 orbitals, d2h, one state", "eps_var": args.eps_var, "device": torch.cuda.get_device_name(0),
       "min_hess": H.ORBOPT_MIN_HESS, "max_step": H.ORBOPT_MAX_STEP, "optimised_orbitals": loop("optimised"), "natural_orbitals": loop("natural")}
if args.solver == "newton":
    doc.update({"cg_tol": H.ORBOPT_CG_TOL, "max_cg": H.ORBOPT_MAX_CG, "newton_orbitals": loop("newton")})
try:
    doc["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    doc["commit"] = None
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
