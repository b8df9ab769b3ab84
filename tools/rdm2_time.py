#!/usr/bin/env python3
"""What the 2-RDM of an HCI wavefunction costs on the device.  One JSON line: the C2 i_1sigma_g wavefunction in the determinant basis
through sqmc_gpu_hci_2rdm one block per call -- wall seconds of every repetition, the HIP-event time of the block's kernels and its
records -- at the deck's eps_var (--eps-var) and at the largest truncation of that list (largest |c| first, sizes doubling from 250)
whose plain evaluation over all pairs, host.two_rdm_host, stays inside --host-budget seconds; that evaluation's seconds; and on the
same run beside them the 1-RDM (with the orbital-symmetry filter, as the deck runs it) and the deterministic PT2 stage at --eps-pt."""
import argparse
import ctypes as C
import copy
import json
import os
import sys
import time

os.environ.setdefault("SQMC_PT2_TIME", "1")
os.environ.setdefault("SQMC_RDM_TIME", "1")
os.environ.setdefault("SQMC_RDM2_TIME", "1")         # read once when the library first runs a 2-RDM: HIP events around a block's kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, default=1e-3)
ap.add_argument("--eps-pt", type=float, default=1e-5, help="threshold of the PT2 stage timed beside the density matrices")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--host-budget", type=float, default=60.0, help="seconds the plain host evaluation may take on the largest list it is given")
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
L.sqmc_gpu_debug_rdm2_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
L.sqmc_gpu_debug_pt2_terms_ms.argtypes = [C.c_void_p, C.c_void_p]
sym = np.asarray(h.orbsym[1:h.norb + 1], np.int32)
med = lambda v: float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def blocks_of(u, d, c):
    """per block: wall seconds and kernel milliseconds of every repetition, records, same bits every time"""
    out = {}
    for k, b in enumerate(("aa", "bb", "ab")):
        gp.two_rdm(u, d, c, b)                        # allocator warm-up
        wall, ms, bits, rec = [], [], set(), 0
        for _ in range(args.repeats):
            dt, m = timed(lambda: gp.two_rdm(u, d, c, b))
            a, r = (C.c_double * 3)(), (C.c_int64 * 3)()
            L.sqmc_gpu_debug_rdm2_ms(gp.h, a, r)
            wall.append(dt); ms.append(a[k]); rec = int(r[k]); bits.add(m[b].tobytes(order="F"))
        out[b] = {"wall_s": wall, "wall_s_median": med(wall), "kernel_ms": ms, "kernel_ms_median": med(ms), "records": rec, "same_bits_every_repeat": len(bits) == 1}
    return out


e0 = float(e[0])
full = blocks_of(du, dd, dc)
gp.one_rdm(du, dd, dc, sym); gp.hci_pt2(du, dd, dc, e0, args.eps_pt)
one, pt2 = [], []
for _ in range(args.repeats):
    dt, m = timed(lambda: gp.one_rdm(du, dd, dc, sym))
    a, b = C.c_double(), C.c_double(); L.sqmc_gpu_debug_rdm_ms(gp.h, C.byref(a), C.byref(b))
    one.append((dt, a.value))
    dt, (de, nconn) = timed(lambda: gp.hci_pt2(du, dd, dc, e0, args.eps_pt))
    ms = C.c_double(); L.sqmc_gpu_debug_pt2_terms_ms(gp.h, C.byref(ms))
    pt2.append((dt, ms.value, de, nconn))
# the host yardstick on truncations by |c|, sizes doubling up to the whole list while the next one is expected to stay inside the budget
order = np.argsort(-np.abs(dc), kind="stable")
n, host_runs, last = min(250, len(dc)), [], None
while True:
    sel = np.sort(order[:n])
    dt, ref = timed(lambda: H.two_rdm_host(du[sel], dd[sel], dc[sel], h.norb))
    host_runs.append({"n": int(n), "seconds": dt})
    last = (sel, ref)
    nxt = min(2 * n, len(dc))
    if n == len(dc) or dt * (nxt / n) ** 2 > args.host_budget:       # all pairs: the next size is expected to take (n_next / n)^2 as long
        break
    n = nxt
sel, ref = last
trunc = blocks_of(du[sel], dd[sel], dc[sel])
dev = gp.two_rdm(du[sel], dd[sel], dc[sel])
gp.close()
print(json.dumps({
    "deck": "C2_r1.24253_i_1sigma_g", "eps_var": args.eps_var, "n_var": int(len(up)), "n_var_determinant_basis": int(len(du)), "e_var": e0, "repeats": args.repeats,
    "two_rdm": full,
    "host_yardstick": {"budget_s": args.host_budget, "runs": host_runs, "n": int(len(sel)), "seconds": host_runs[-1]["seconds"], "two_rdm_on_that_list": trunc,
                       "max_abs_difference_device_host": max(float(np.max(np.abs(dev[b] - ref[b]))) for b in dev)},
    "one_rdm": {"wall_s_median": med([r[0] for r in one]), "kernel_ms_median": med([r[1] for r in one])},
    "pt2": {"eps_pt": args.eps_pt, "wall_s_median": med([r[0] for r in pt2]), "term_kernel_ms_median": med([r[1] for r in pt2]), "delta_e": pt2[0][2], "n_connections": int(pt2[0][3])},
}))
