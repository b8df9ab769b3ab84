#!/usr/bin/env python3
"""What an orbital Hessian-vector product costs on the device.  Writes one JSON document (default profiles/orbhess_time.json) with a
record per case:

  26       the C2 fixture: the density matrices of the eps_var 5e-3 wavefunction (state 1 of two), kappa from host.orbital_step;
  32, 64   dense random integrals in the identity pair order, a random symmetric D, a G with the symmetries of a real one, a random
           antisymmetric kappa.

Per record, medians of --repeats: HIP-event milliseconds of the four stages of a product (the half pass of the one-index
transformation, its symmetrising pass with the one-body block, the Fock GEMM on the transformed table with its reduction, the sigma
kernel; SQMC_ORBHESS_TIME); wall milliseconds of OrbOptPlan.hessian_vector and of building the plan; and -- the comparisons, not the
code under test -- wall milliseconds of the same product the way it had to be done without the plan (host.one_index_transform_host,
packing, a new context on the transformed table, GpuChem.orbital_gradient, the commutator in numpy) and of
host.orbital_hessian_vector_host, each with its largest difference from the plan's product."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("SQMC_ORBHESS_TIME", "1")      # read once when the library first runs a product: HIP events around its stages
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--eps-var", type=float, default=5e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbhess_time.json"))
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_orbhess_ms.argtypes = [C.c_void_p, C.c_void_p]
L.sqmc_gpu_debug_orbhess_plan.argtypes = [C.c_int32, C.c_void_p]
med = lambda v: float(np.median(v))
STAGES = ("half_pass", "symmetrise_and_one_body", "fock_on_transformed_table", "sigma")


def pack_index(n, c2):
    n1 = n + 1
    pr = c2[1:n1, 1:n1].astype(np.int64)
    hi, lo = np.maximum(pr[:, :, None, None], pr[None, None, :, :]), np.minimum(pr[:, :, None, None], pr[None, None, :, :])
    A = int(c2[n1, n1])
    return (hi * (hi - 1)) // 2 + lo, A * (A - 1) // 2 + pr


def measure(g, host, D, G, kappa, context_on):
    """context_on(packed): a new context on another packed table with g's geometry"""
    n = g.norb
    t0 = time.perf_counter()
    plan = g.orbopt_plan(D, G)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    plan.hessian_vector(kappa)        # allocator and code-object warm-up
    wall, ker, bits = [], [], set()
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        sig = plan.hessian_vector(kappa)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = (C.c_double * 4)()
        L.sqmc_gpu_debug_orbhess_ms(plan.h, ms)
        ker.append(tuple(ms)); bits.add(sig.tobytes())
    grad = plan.gradient("gradient")["gradient"]
    plan.close()
    # the way without the plan
    i2, i1 = pack_index(n, host.combine_2)
    old = []
    for _ in range(max(2, args.repeats // 2)):
        t0 = time.perf_counter()
        ht, et = H.one_index_transform_host(host, kappa)
        packed = np.zeros_like(host.integrals)
        packed[i2] = et; packed[i1] = ht
        g2 = context_on(packed)
        try:
            gt = g2.orbital_gradient(D, G, "gradient")["gradient"]
        finally:
            g2.close()
        g0 = g.orbital_gradient(D, G, "gradient")["gradient"]
        sig_old = gt + 0.5 * (kappa @ g0 - g0 @ kappa)
        old.append(1e3 * (time.perf_counter() - t0))
    hw = []
    for _ in range(2):
        t0 = time.perf_counter()
        ref = H.orbital_hessian_vector_host(host, D, G, kappa)
        hw.append(1e3 * (time.perf_counter() - t0))
    shape = (C.c_int64 * 4)()
    L.sqmc_gpu_debug_orbhess_plan(n, shape)
    npair = shape[2]
    rec = {"norb": n, "repeats": args.repeats, "half_pass_register_tile": shape[0], "symmetrising_tile": shape[1], "pairs": npair, "symmetrising_blocks": shape[3],
           "half_pass_lds_bytes_per_block": 16 * n * n, "half_pass_gathered_doubles": npair * n * n, "half_pass_fma": 2 * npair * npair * n,
           "work_buffer_bytes": 8 * npair * npair}
    for j, name in enumerate(STAGES):
        rec["kernel_ms_%s_median" % name] = med([k[j] for k in ker])
        rec["kernel_ms_%s" % name] = [k[j] for k in ker]
    half = rec["kernel_ms_half_pass_median"]
    rec.update({"half_pass_gflops_fp64": 2e-6 * rec["half_pass_fma"] / half if half > 0 else None,
                "half_pass_gather_gbytes_per_s": 8e-6 * rec["half_pass_gathered_doubles"] / half if half > 0 else None,
                "plan_prepare_wall_ms": plan_ms, "product_wall_ms": wall, "product_wall_ms_median": med(wall), "same_bits_every_repeat": len(bits) == 1,
                "without_plan_wall_ms": old, "without_plan_wall_ms_median": med(old), "max_abs_difference_from_without_plan": float(np.max(np.abs(sig - sig_old))),
                "host_numpy_wall_ms": hw, "max_abs_difference_from_host": float(np.max(np.abs(sig - ref))), "max_abs_sigma": float(np.max(np.abs(sig))),
                "max_abs_gradient": float(np.max(np.abs(grad)))})
    return rec


records = []
# ---- C2
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, w, e, _ = H.hci_variational(h, g, args.eps_var, n_states=2, max_iters=1)
w = np.asarray(w, float).reshape(len(up), -1)
D = H.hci_one_rdm(h, up, dn, w[:, 0])
G = H.spin_free_two_rdm(H.hci_two_rdm(h, up, dn, w[:, 0]))
og = g.orbital_gradient(D, G)
kappa = H.orbital_step(og["gradient"], og["hdiag"], h.orbsym[1:h.norb + 1])
rec = measure(g, h, D, G, kappa, lambda packed: h.with_integrals(packed).gpu())
g.close()
rec["system"] = "C2_r1.24253 cc-pVDZ, state 1 of the eps_var %g wavefunction (two states, one iteration), %d determinants; kappa of host.orbital_step" % (args.eps_var, len(up))
records.append(rec)
print(json.dumps(rec), flush=True)

# ---- 32 and 64 orbitals: dense random integrals
for n in (32, 64):
    rng = np.random.default_rng(n)
    n1 = n + 1
    c2 = np.zeros((n + 2, n + 2), np.int32)
    i, j = np.meshgrid(np.arange(1, n1), np.arange(1, n1), indexing="ij")
    c2[1:n1, 1:n1] = (np.maximum(i, j) * (np.maximum(i, j) - 1)) // 2 + np.minimum(i, j)
    A = (n1 * n) // 2 + n1
    c2[n1, n1] = A
    packed = rng.uniform(-1.0, 1.0, A * (A - 1) // 2 + A + 1)
    packed[0] = 0.0
    prod = np.zeros((9, 9), np.int32); prod[1, 1] = 1
    make = lambda tab: sqmc_amd.GpuChem(n, 1, 1, np.ones(n1, np.int32), prod.reshape(-1), c2.reshape(-1), tab, n_group=1)
    g = make(packed)
    host = H.ChemHost.__new__(H.ChemHost)              # what dense_integrals reads, nothing else
    host.norb, host.combine_2, host.integrals = n, c2, packed
    D = rng.uniform(-1.0, 1.0, (n, n)); D = D + D.T
    G = rng.uniform(-1.0, 1.0, (n,) * 4)
    G = G + G.transpose(2, 3, 0, 1); G = G + G.transpose(1, 0, 3, 2)
    kappa = np.triu(rng.uniform(-1.0, 1.0, (n, n)), 1); kappa = kappa - kappa.T
    rec = measure(g, host, D, G, kappa, make)
    g.close()
    rec["system"] = "dense random integrals, random symmetric D, G with G[pqrs] = G[rspq] = G[qpsr], random antisymmetric kappa"
    records.append(rec)
    print(json.dumps(rec), flush=True)

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    commit = None
doc = {"tool": "tools/orbhess_time.py", "command": "python tools/orbhess_time.py --repeats %d --eps-var %g" % (args.repeats, args.eps_var),
       "commit": commit, "device": torch.cuda.get_device_name(0), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
