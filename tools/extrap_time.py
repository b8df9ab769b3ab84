#!/usr/bin/env python3
"""What a truncation's Hamiltonian costs in the energies for extrapolation (host.hci_extrapolation_energies): extracted from the whole
list's resident plan (sqmc_gpu_spmv_plan_submatrix) against built from its determinants (sqmc_gpu_build_spmv_plan), beside the
Davidson run and the PT stage the truncation needs anyway.  Prints one JSON line and writes it to profiles/extrap_time.json: the C2
i_1sigma_g wavefunction (one state) at --eps-var, --n-energy-batch truncations, and per truncation the host-clock wall seconds of
SpmvPlan.submatrix with the HIP-event times of its kernels (mark + count + scan; fill), the wall seconds of SpmvPlan.from_dets on the
same subset -- both the median of --repeats calls after one warm-up call --, whether the two plans multiply to the same bits, the
products and the wall seconds of the Davidson run, and the wall seconds of the deterministic PT stage at --eps-pt (one call)."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("SQMC_SUBMATRIX_TIME", "1")      # read once when the library first extracts a submatrix: HIP events around its kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, default=1e-4)
ap.add_argument("--n-energy-batch", type=int, default=10)
ap.add_argument("--eps-pt", type=float, default=1e-7, help="threshold of the deterministic PT stage (the shipped deck's)")
ap.add_argument("--pt-slices", type=int, default=1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extrap_time.json"))
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_submatrix_ms.argtypes = [C.c_void_p, C.c_void_p]
med = lambda v: float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, wts, e, hist = H.hci_variational(h, g, args.eps_var, eps_sched=(2 * args.eps_var, 2 * args.eps_var))
n = len(up)
plain = copy.copy(h); plain.time_sym = False
gp = plain.gpu()
gp.set_hb_tables(*plain.hb_tables(gp))

iorder, w = H.extrapolation_order(wts)
order_full = H.sort_dets(up, dn)
t_full, (full, diag_full, nnz_full) = timed(lambda: sqmc_amd.SpmvPlan.from_dets(g, up[order_full], dn[order_full]))
rank = np.empty(n, np.int64); rank[order_full] = np.arange(n)
up_m, dn_m = up[iorder], dn[iorder]
rows = []
for nt, printed in H.extrapolation_truncations(n, args.n_energy_batch):
    o = H.sort_dets(up_m[:nt], dn_m[:nt])
    tu, td, v0 = up_m[:nt][o], dn_m[:nt][o], w[:nt][o]
    sel = rank[iorder[:nt][o]]
    full.submatrix(sel).close()
    sub_t = []
    for _ in range(args.repeats):
        dt, sub = timed(lambda: full.submatrix(sel))
        a, b = C.c_double(), C.c_double()
        L.sqmc_gpu_debug_submatrix_ms(C.byref(a), C.byref(b))
        sub_t.append((dt, a.value, b.value))
        sub.close()
    sqmc_amd.SpmvPlan.from_dets(g, tu, td)[0].close()
    build_t = []
    for _ in range(args.repeats):
        dt, (ref, dref, nnz) = timed(lambda: sqmc_amd.SpmvPlan.from_dets(g, tu, td))
        build_t.append(dt)
        ref.close()
    sub = full.submatrix(sel)
    ref, dref, nnz = sqmc_amd.SpmvPlan.from_dets(g, tu, td)
    x = np.random.default_rng(nt).standard_normal(nt)
    same = sub.apply(x).tobytes() == ref.apply(x).tobytes() and np.array_equal(dref, diag_full[sel]) and (sub.nnz_full + nt) // 2 == nnz
    ref.close()
    t_dav, (ev, X, n_mv) = timed(lambda: sub.davidson(diag_full[sel], k=1, v0=v0, tol=1e-10))
    sub.close()
    du, dd, dc = H.time_symmetrized_to_dets(tu, td, X[:, 0], h.z)
    slices = args.pt_slices
    while True:                                     # connections that do not fit one call: more slices of the key range, which is exact
        try:
            t_pt, (de, nconn) = timed(lambda: gp.hci_pt2(du, dd, dc, float(ev[0]), args.eps_pt, slices))
            break
        except sqmc_amd.SqmcGpuError:
            if slices >= 64:
                raise
            slices *= 4
    rows.append({"ndets": int(nt), "ndets_printed": int(printed), "ndets_determinant_basis": int(len(du)), "nnz_upper": int(nnz), "nnz_full": int(2 * nnz - nt),
                 "submatrix_wall_s": [r[0] for r in sub_t], "submatrix_wall_s_median": med([r[0] for r in sub_t]),
                 "submatrix_count_scan_ms_median": med([r[1] for r in sub_t]), "submatrix_fill_ms_median": med([r[2] for r in sub_t]),
                 "from_dets_wall_s": build_t, "from_dets_wall_s_median": med(build_t),
                 "submatrix_over_from_dets": med([r[0] for r in sub_t]) / med(build_t), "same_plan": bool(same),
                 "davidson_matvecs": int(n_mv), "davidson_wall_s": t_dav, "e_var": float(ev[0]),
                 "pt_wall_s": t_pt, "pt_slices": slices, "pt_delta_e": float(de), "pt_connected": int(nconn)})
full.close(); gp.close(); g.close()
out = {"deck": "C2_r1.24253_i_1sigma_g", "n_states": 1, "eps_var": args.eps_var, "eps_pt": args.eps_pt, "n_energy_batch": args.n_energy_batch,
       "repeats": args.repeats, "ndets": int(n), "nnz_upper_full_space": int(nnz_full), "from_dets_full_space_wall_s": t_full, "e_var_full_space": float(e[0]),
       "submatrix_faster_at_every_truncation": bool(all(r["submatrix_over_from_dets"] < 1.0 for r in rows)), "truncations": rows}
print(json.dumps(out), flush=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
