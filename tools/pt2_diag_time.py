#!/usr/bin/env python3
"""What the O(N) diagonal update (get_new_diag_elem, sqmc_gpu_hci_set_diag_update) is worth in the deterministic PT2 stage.
One JSON line: the PT2 stage of the C2 i_1sigma_g deck (eps_var 1e-4, eps_pt 1e-6, as tools/bench_hci.py runs it: determinant
basis, one slice) in modes 0, 1 and 2 -- wall seconds of every repetition, their median and scatter, the HIP-event time of the
term kernel (membership search + H_aa + term: the kernel the mode changes), delta_E_PT and the connection count per mode.
On a checkout that has no update (the parent of the change that added it) only mode 0 is run and no kernel time is reported:
run it there with --repeats 5, keep the line, and hand it to the run on the new build with --parent FILE; the output then carries
the parent's times and scatter beside the three modes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("SQMC_PT2_TIME", "1")          # read once when the library first runs a PT2: HIP events around the term kernel
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, default=1e-4)
ap.add_argument("--eps-pt", type=float, default=1e-6)
ap.add_argument("--pt-slices", type=int, default=1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--parent", default=None, help="the JSON line of this tool run on the parent commit")
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, w, e, hist = H.hci_variational(h, g, args.eps_var, eps_sched=(2 * args.eps_var, 2 * args.eps_var))
g.close()
import copy      # noqa: E402
plain = copy.copy(h); plain.time_sym = False
du, dd, dc = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
gp = plain.gpu()
gp.set_hb_tables(*plain.hb_tables(gp))
L = sqmc_amd.load_library()
has_update = hasattr(gp, "hci_set_diag_update")
has_timer = hasattr(L, "sqmc_gpu_debug_pt2_terms_ms")


def stage(mode):
    t0 = time.perf_counter()
    if has_update:
        de, n = H.hci_pt2(plain, gp, du, dd, dc, float(e[0]), args.eps_pt, args.pt_slices, diag_update=mode)
    else:
        de, n = H.hci_pt2(plain, gp, du, dd, dc, float(e[0]), args.eps_pt, args.pt_slices)
    dt = time.perf_counter() - t0
    ms = C.c_double(float("nan"))
    if has_timer:
        L.sqmc_gpu_debug_pt2_terms_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.sqmc_gpu_debug_pt2_terms_ms(gp.h, C.byref(ms))
    return dt, ms.value, de, n


out = {"deck": "C2_r1.24253_i_1sigma_g", "eps_var": args.eps_var, "eps_pt": args.eps_pt, "pt_slices": args.pt_slices, "n_var": int(len(up)),
       "n_var_determinant_basis": int(len(du)), "e_var": float(e[0]), "repeats": args.repeats, "modes": {}}
stage(0)                                             # first call: allocator warm-up, not timed
for mode in ((0, 1, 2) if has_update else (0,)):
    runs = [stage(mode) for _ in range(args.repeats)]
    ts = np.array([r[0] for r in runs]); ks = np.array([r[1] for r in runs])
    out["modes"][str(mode)] = {"pt2_s": [float(x) for x in ts], "pt2_s_median": float(np.median(ts)), "pt2_s_min": float(ts.min()),
                               "pt2_s_scatter": float((ts.max() - ts.min()) / np.median(ts)),
                               "term_kernel_ms": None if not has_timer else [float(x) for x in ks],
                               "term_kernel_ms_median": None if not has_timer else float(np.median(ks)),
                               "delta_e_pt": runs[0][2], "n_connections": int(runs[0][3]), "same_bits_every_repeat": len({r[2] for r in runs}) == 1}
gp.close()
if args.parent:
    with open(args.parent) as f:
        par = json.loads([l for l in f.read().splitlines() if l.startswith("{")][-1])
    p0, m0 = par["modes"]["0"], out["modes"]["0"]
    out["parent"] = {"pt2_s": p0["pt2_s"], "pt2_s_median": p0["pt2_s_median"], "pt2_s_scatter": p0["pt2_s_scatter"], "delta_e_pt": p0["delta_e_pt"],
                     "n_connections": p0["n_connections"]}
    out["mode0_over_parent"] = m0["pt2_s_median"] / p0["pt2_s_median"]
    out["mode0_within_parent_scatter"] = bool(abs(m0["pt2_s_median"] - p0["pt2_s_median"]) <= p0["pt2_s_scatter"] * p0["pt2_s_median"])
    out["mode0_same_bits_as_parent"] = bool(m0["delta_e_pt"] == p0["delta_e_pt"] and m0["n_connections"] == p0["n_connections"])
print(json.dumps(out))
