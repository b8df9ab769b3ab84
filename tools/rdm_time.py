#!/usr/bin/env python3
"""What the 1-RDM of an HCI wavefunction costs on the device.  One JSON line: the C2 i_1sigma_g wavefunction at eps_var 1e-4 in the
determinant basis (the wavefunction of profiles/pt2_diag_update.json) through sqmc_gpu_hci_1rdm (with the orbital-symmetry filter,
as the deck runs it) and sqmc_gpu_hci_1rdm_pt at --eps-pt-big -- wall seconds of every repetition and the HIP-event time of their
kernels (variational pass; psi1 + PT pass + sums over all slices) -- and, on the same run beside them, the deterministic PT2 stage
at the same threshold (wall seconds, HIP-event time of its term kernel)."""
import argparse
import ctypes as C
import copy
import json
import os
import sys
import time

os.environ.setdefault("SQMC_PT2_TIME", "1")
os.environ.setdefault("SQMC_RDM_TIME", "1")          # read once when the library first runs a 1-RDM: HIP events around its kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, default=1e-4)
ap.add_argument("--eps-pt-big", type=float, default=1e-5, help="threshold of the connected space of the PT-corrected 1-RDM and of the PT2 stage beside it")
ap.add_argument("--pt-slices", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, w, e, hist = H.hci_variational(h, g, args.eps_var, eps_sched=(2 * args.eps_var, 2 * args.eps_var))
g.close()
plain = copy.copy(h); plain.time_sym = False
du, dd, dc = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
gp = plain.gpu()
gp.set_hb_tables(*plain.hb_tables(gp))
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_rdm_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
L.sqmc_gpu_debug_pt2_terms_ms.argtypes = [C.c_void_p, C.c_void_p]
sym = np.asarray(h.orbsym[1:h.norb + 1], np.int32)


def kernel_ms():
    a, b = C.c_double(), C.c_double()
    L.sqmc_gpu_debug_rdm_ms(gp.h, C.byref(a), C.byref(b))
    return a.value, b.value


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


e0 = float(e[0])
gp.one_rdm(du, dd, dc, sym); gp.one_rdm_pt(du, dd, dc, e0, args.eps_pt_big, args.pt_slices); gp.hci_pt2(du, dd, dc, e0, args.eps_pt_big, args.pt_slices)      # allocator warm-up
var, pt, pt2 = [], [], []
for _ in range(args.repeats):
    dt, m = timed(lambda: gp.one_rdm(du, dd, dc, sym))
    var.append((dt, kernel_ms()[0], m.tobytes()))
    dt, (m, nconn) = timed(lambda: gp.one_rdm_pt(du, dd, dc, e0, args.eps_pt_big, args.pt_slices))
    pt.append((dt, kernel_ms(), m.tobytes(), nconn, float(np.trace(m)), float(np.max(np.abs(m - m.T)))))
    dt, (de, n2) = timed(lambda: gp.hci_pt2(du, dd, dc, e0, args.eps_pt_big, args.pt_slices))
    ms = C.c_double(); L.sqmc_gpu_debug_pt2_terms_ms(gp.h, C.byref(ms))
    pt2.append((dt, ms.value, de, n2))
gp.close()
med = lambda v: float(np.median(v))
print(json.dumps({
    "deck": "C2_r1.24253_i_1sigma_g", "eps_var": args.eps_var, "eps_pt_big": args.eps_pt_big, "pt_slices": args.pt_slices, "n_var": int(len(up)),
    "n_var_determinant_basis": int(len(du)), "e_var": e0, "repeats": args.repeats,
    "one_rdm": {"wall_s": [r[0] for r in var], "wall_s_median": med([r[0] for r in var]), "kernel_ms": [r[1] for r in var], "kernel_ms_median": med([r[1] for r in var]),
                "same_bits_every_repeat": len({r[2] for r in var}) == 1},
    "one_rdm_pt": {"wall_s": [r[0] for r in pt], "wall_s_median": med([r[0] for r in pt]), "variational_kernel_ms_median": med([r[1][0] for r in pt]),
                   "pt_kernels_ms": [r[1][1] for r in pt], "pt_kernels_ms_median": med([r[1][1] for r in pt]), "n_connections": int(pt[0][3]), "trace": pt[0][4],
                   "max_asymmetry": pt[0][5], "same_bits_every_repeat": len({r[2] for r in pt}) == 1},
    "pt2_stage": {"wall_s": [r[0] for r in pt2], "wall_s_median": med([r[0] for r in pt2]), "term_kernel_ms_median": med([r[1] for r in pt2]), "delta_e_pt": pt2[0][2],
                  "n_connections": int(pt2[0][3])}}))
