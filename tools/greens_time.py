#!/usr/bin/env python3
"""What the zeroth-order Green's function of an HCI wavefunction costs on the device.  Writes profiles/greens_time.json: the C2
i_1sigma_g wavefunctions at eps_var 1e-3 and 1e-4 (time-symmetrised, expanded in determinants as host.hci_greens_function expands
them) through sqmc_gpu_hci_greens_function at n_w = 20 and 200 on the deck's kind of uniform grid -- host-clock wall seconds of the
synchronous call and the HIP-event times of its pole passes and term passes -- and beside them, on the same machine,
host.greens_function_host on the same input and the deterministic PT2 stage of the same wavefunction at --eps-pt.  Every figure is
the median of --repeats calls after one warm-up call."""
import argparse
import ctypes as C
import copy
import json
import os
import sys
import time

os.environ.setdefault("SQMC_GREENS_TIME", "1")       # read once when the library first runs a Green's function: HIP events around its passes
os.environ.setdefault("SQMC_PT2_TIME", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, nargs="+", default=[1e-3, 1e-4])
ap.add_argument("--n-w", type=int, nargs="+", default=[20, 200])
ap.add_argument("--w-min", type=float, default=-1.0)
ap.add_argument("--w-max", type=float, default=1.0)
ap.add_argument("--eps-pt", type=float, default=1e-5, help="threshold of the deterministic PT2 stage timed beside the Green's function")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--host-repeats", type=int, default=None, help="repetitions of greens_function_host (default: --repeats)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greens_time.json"))
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_greens_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
L.sqmc_gpu_debug_pt2_terms_ms.argtypes = [C.c_void_p, C.c_void_p]
med = lambda v: float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


cases = []
for eps_var in args.eps_var:
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    g = h.gpu()
    g.set_hb_tables(*h.hb_tables(g))
    up, dn, wts, e, hist = H.hci_variational(h, g, eps_var, eps_sched=(2 * eps_var, 2 * eps_var))
    g.close()
    plain = copy.copy(h); plain.time_sym = False
    du, dd, dc = H.time_symmetrized_to_dets(up, dn, wts[:, 0], h.z)
    e0 = float(e[0])
    gp = plain.gpu()
    gp.set_hb_tables(*plain.hb_tables(gp))
    gp.hci_pt2(du, dd, dc, e0, args.eps_pt)
    pt2 = []
    for _ in range(args.repeats):
        dt, (de, nconn) = timed(lambda: gp.hci_pt2(du, dd, dc, e0, args.eps_pt))
        ms = C.c_double(); L.sqmc_gpu_debug_pt2_terms_ms(gp.h, C.byref(ms))
        pt2.append((dt, ms.value, de, nconn))
    for n_w in args.n_w:
        w = H.greens_grid(n_w, args.w_min, args.w_max)
        gp.greens_function(du, dd, dc, e0, w)
        devt, bits = [], set()
        for _ in range(args.repeats):
            dt, (a, b) = timed(lambda: gp.greens_function(du, dd, dc, e0, w))
            p_ms, t_ms = C.c_double(), C.c_double()
            L.sqmc_gpu_debug_greens_ms(gp.h, C.byref(p_ms), C.byref(t_ms))
            devt.append((dt, p_ms.value, t_ms.value)); bits.add(a.tobytes() + b.tobytes())
        H.greens_function_host(plain, du, dd, dc, e0, w)
        hostt = []
        for _ in range(args.host_repeats or args.repeats):
            dt, (ha, hb) = timed(lambda: H.greens_function_host(plain, du, dd, dc, e0, w))
            hostt.append(dt)
        scale = max(float(np.max(np.abs(a))), float(np.max(np.abs(b))))
        cases.append({"eps_var": eps_var, "n_var": int(len(up)), "n_var_determinant_basis": int(len(du)), "e_var": e0, "n_w": n_w, "w_min": args.w_min, "w_max": args.w_max,
                      "device": {"wall_s": [r[0] for r in devt], "wall_s_median": med([r[0] for r in devt]), "pole_passes_ms_median": med([r[1] for r in devt]),
                                 "term_passes_ms_median": med([r[2] for r in devt]), "same_bits_every_repeat": len(bits) == 1},
                      "host": {"wall_s": hostt, "wall_s_median": med(hostt)},
                      "device_over_host": med([r[0] for r in devt]) / med(hostt),
                      "max_abs_difference_device_host": max(float(np.max(np.abs(a - ha))), float(np.max(np.abs(b - hb)))), "max_abs_entry": scale,
                      "pt2_stage": {"eps_pt": args.eps_pt, "wall_s_median": med([r[0] for r in pt2]), "term_kernel_ms_median": med([r[1] for r in pt2]), "delta_e_pt": pt2[0][2],
                                    "n_connections": int(pt2[0][3])}})
        print(json.dumps(cases[-1]), flush=True)
    gp.close()
with open(args.out, "w") as f:
    json.dump({"deck": "C2_r1.24253_i_1sigma_g", "repeats": args.repeats, "host_repeats": args.host_repeats or args.repeats, "cases": cases}, f, indent=1)
    f.write("\n")
