#!/usr/bin/env python3
"""What the two-body transition density matrix of two HCI vectors costs on the device, beside the 2-RDM on the same list.  Writes one
JSON document (default profiles/tdm_time.json).  Two lists: the C2 i_1sigma_g wavefunction with two states in the determinant basis
(bra = state 1, ket = state 2) at --eps-var, and a dense 64-orbital case (the 8 x 8 Hubbard lattice, 3 up and 2 dn electrons,
--n-dense determinants grown by single moves, random vectors).  Per list and block, one block per call: wall seconds and the
HIP-event time of the block's kernels for two_tdm and for two_rdm, the polarisation route [two_rdm(b + k) - two_rdm(b - k)] / 4 (two
2-RDM calls plus numpy: it gives the symmetrised matrix only), and host.two_tdm_host on the largest truncation (sizes doubling from
250) that stays inside --host-budget seconds."""
import argparse
import ctypes as C
import copy
import json
import os
import random
import sys
import time

os.environ.setdefault("SQMC_RDM2_TIME", "1")         # read once when the library first runs a block: HIP events around its kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--eps-var", type=float, default=1e-3)
ap.add_argument("--n-dense", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--host-budget", type=float, default=60.0, help="seconds the plain host evaluation may take on the largest list it is given")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdm_time.json"))
args = ap.parse_args()

sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_rdm2_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
med = lambda v: float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def kernel_ms(g, k):
    a, r = (C.c_double * 3)(), (C.c_int64 * 3)()
    L.sqmc_gpu_debug_rdm2_ms(g.h, a, r)
    return a[k], int(r[k])


def measure(g, u, d, bra, ket):
    """per block: two_tdm, two_rdm(ket) and the polarisation route, wall and kernel times of every repetition"""
    out = {}
    plus, minus = bra + ket, bra - ket
    for k, b in enumerate(("aa", "bb", "ab")):
        g.two_tdm(u, d, bra, ket, b); g.two_rdm(u, d, ket, b)      # allocator warm-up
        rows = {"two_tdm": ([], []), "two_rdm": ([], []), "polarisation": ([], [])}
        bits, rec, worst = set(), 0, 0.0
        for _ in range(args.repeats):
            dt, t = timed(lambda: g.two_tdm(u, d, bra, ket, b))
            ms, rec = kernel_ms(g, k)
            rows["two_tdm"][0].append(dt); rows["two_tdm"][1].append(ms); bits.add(t[b].tobytes(order="F"))
            dt, _ = timed(lambda: g.two_rdm(u, d, ket, b))
            rows["two_rdm"][0].append(dt); rows["two_rdm"][1].append(kernel_ms(g, k)[0])
            t0 = time.perf_counter()
            gp_ = g.two_rdm(u, d, plus, b)[b]; ms1 = kernel_ms(g, k)[0]
            gm_ = g.two_rdm(u, d, minus, b)[b]; ms2 = kernel_ms(g, k)[0]
            pol = (gp_ - gm_) / 4
            rows["polarisation"][0].append(time.perf_counter() - t0); rows["polarisation"][1].append(ms1 + ms2)
            worst = max(worst, float(np.max(np.abs(pol - (t[b] + t[b].transpose(2, 3, 0, 1)) / 2))))
            del gp_, gm_, pol, t
        out[b] = {name: {"wall_s": w, "wall_s_median": med(w), "kernel_ms": m, "kernel_ms_median": med(m)} for name, (w, m) in rows.items()}
        out[b].update(records=rec, same_bits_every_repeat=len(bits) == 1, max_abs_difference_polarisation_symmetrised=worst,
                      kernel_ratio_tdm_over_rdm=med(rows["two_tdm"][1]) / med(rows["two_rdm"][1]) if med(rows["two_rdm"][1]) > 0 else None,
                      wall_ratio_tdm_over_rdm=med(rows["two_tdm"][0]) / med(rows["two_rdm"][0]))
    return out


def host_yardstick(g, u, d, bra, ket, norb):
    order = np.argsort(-np.abs(bra) - np.abs(ket), kind="stable")
    n, runs, last = min(250, len(bra)), [], None
    while True:
        sel = np.sort(order[:n])
        dt, ref = timed(lambda: H.two_tdm_host(u[sel], d[sel], bra[sel], ket[sel], norb, "ab"))
        runs.append({"n": int(n), "seconds": dt})
        last = (sel, ref)
        nxt = min(2 * n, len(bra))
        if n == len(bra) or dt * (nxt / n) ** 2 > args.host_budget:      # all pairs: the next size is expected to take (n_next / n)^2 as long
            break
        n = nxt
    sel, ref = last
    dt, dev = timed(lambda: g.two_tdm(u[sel], d[sel], bra[sel], ket[sel], "ab"))
    return {"budget_s": args.host_budget, "block": "ab", "runs": runs, "n": int(len(sel)), "seconds": runs[-1]["seconds"], "two_tdm_wall_s_on_that_list": dt,
            "max_abs_difference_device_host": float(np.max(np.abs(dev["ab"] - ref["ab"])))}


FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, w, e, hist = H.hci_variational(h, g, args.eps_var, eps_sched=(2 * args.eps_var, 2 * args.eps_var), n_states=2)
g.close()
plain = copy.copy(h); plain.time_sym = False
du, dd, c0 = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
_, _, c1 = H.time_symmetrized_to_dets(up, dn, w[:, 1], h.z)
gp = plain.gpu()
c2 = {"deck": "C2_r1.24253_i_1sigma_g", "eps_var": args.eps_var, "n_var": int(len(up)), "n_var_determinant_basis": int(len(du)), "norb": h.norb,
      "blocks": measure(gp, du, dd, c0, c1), "host_yardstick": host_yardstick(gp, du, dd, c0, c1, h.norb)}
gp.close()

hh = H.HubbardHost(8, 8, True, 3, 2)
gh = hh.gpu()
rng = random.Random(64)
have, lst = {(int(hh.hf_up), int(hh.hf_dn))}, [(int(hh.hf_up), int(hh.hf_dn))]
while len(lst) < args.n_dense:
    u_, d_ = lst[rng.randrange(len(lst))]
    spin = rng.randrange(2)
    s = d_ if spin else u_
    occ = [k for k in range(64) if s >> k & 1]
    s2 = (s ^ (1 << rng.choice(occ))) | (1 << rng.choice([k for k in range(64) if not s >> k & 1]))
    det = (u_, s2) if spin else (s2, d_)
    if det not in have:
        have.add(det); lst.append(det)
hu, hd = np.array([x[0] for x in lst], np.uint64), np.array([x[1] for x in lst], np.uint64)
rs = np.random.RandomState(64)
b64, k64 = rs.uniform(-1, 1, len(lst)), rs.uniform(-1, 1, len(lst))
b64, k64 = b64 / np.linalg.norm(b64), k64 / np.linalg.norm(k64)
dense = {"system": "hubbard 8 x 8, 3 up 2 dn", "n": len(lst), "norb": 64, "blocks": measure(gh, hu, hd, b64, k64)}
gh.close()

doc = {"repeats": args.repeats, "c2": c2, "dense64": dense}
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps({b: {"c2_kernel_ratio": c2["blocks"][b]["kernel_ratio_tdm_over_rdm"], "dense64_kernel_ratio": dense["blocks"][b]["kernel_ratio_tdm_over_rdm"]} for b in ("aa", "bb", "ab")}))
