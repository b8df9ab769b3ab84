#!/usr/bin/env python3
"""What the orbital gradient costs on the device.  Writes one JSON document (default profiles/orbopt_time.json) with a record per case:

  26       the C2 fixture: the density matrices of the eps_var 5e-3 wavefunction (state 1 of two);
  32, 64   dense random integrals in the identity pair order, a random symmetric D and a G with the symmetries of a real one.

Per record: HIP-event milliseconds of the kernels (the Fock GEMM with its reduction, the gradient, the diagonal Hessian;
SQMC_ORBOPT_TIME), wall milliseconds of the sqmc_gpu_orbital_gradient call (finite check and upload of norb^4 doubles, allocation,
kernels, copy back), and -- the comparison, not the code under test -- wall milliseconds of host.orbital_gradient_host (numpy einsum on
the unpacked norb^4 integrals, unpacking included) with the largest difference between the two.  For C2 also the wall time of the
2-RDM (host.hci_two_rdm), of the 1-RDM and of one rotation (GpuChem.rotate_integrals) beside it."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("SQMC_ORBOPT_TIME", "1")       # read once when the library first runs the door: HIP events around its kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--eps-var", type=float, default=5e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbopt_time.json"))
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_orbopt_ms.argtypes = [C.c_void_p] * 4
L.sqmc_gpu_debug_orbopt_plan.argtypes = [C.c_int32, C.c_void_p]
med = lambda v: float(np.median(v))


def kernel_ms(g):
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    L.sqmc_gpu_debug_orbopt_ms(g.h, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def measure(g, host, D, G):
    n = g.norb
    g.orbital_gradient(D, G)          # allocator and code-object warm-up
    wall, ker, bits = [], [], set()
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = g.orbital_gradient(D, G)
        wall.append(1e3 * (time.perf_counter() - t0))
        ker.append(kernel_ms(g)); bits.add(b"".join(out[k].tobytes() for k in sorted(out)))
    hw = []
    for _ in range(2):
        t0 = time.perf_counter()
        ref = H.orbital_gradient_host(host, D, G)
        hw.append(1e3 * (time.perf_counter() - t0))
    plan = (C.c_int64 * 4)()
    L.sqmc_gpu_debug_orbopt_plan(n, plan)
    fma = n ** 5 + n ** 3
    fock = med([k[0] for k in ker])
    return {"norb": n, "repeats": args.repeats, "fock_register_tile": plan[0], "fock_triples_per_chunk": plan[1], "fock_chunks_per_block": plan[2], "fock_blocks": plan[3],
            "kernel_ms_fock_median": fock, "kernel_ms_gradient_median": med([k[1] for k in ker]), "kernel_ms_hdiag_median": med([k[2] for k in ker]),
            "kernel_ms_fock": [k[0] for k in ker], "kernel_ms_hdiag": [k[2] for k in ker], "fock_fma": fma,
            "fock_gflops_fp64": 2e-6 * fma / fock if fock > 0 else None,
            "abi_call_wall_ms": wall, "abi_call_wall_ms_median": med(wall), "same_bits_every_repeat": len(bits) == 1,
            "host_einsum_wall_ms": hw, "max_abs_difference_from_host": {k: float(np.max(np.abs(out[k] - ref[k]))) for k in out},
            "max_abs_fock": float(np.max(np.abs(out["fock"])))}


records = []
# ---- C2
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", hf_symmetry=1)
g = h.gpu()
g.set_hb_tables(*h.hb_tables(g))
up, dn, w, e, _ = H.hci_variational(h, g, args.eps_var, n_states=2, max_iters=1)
w = np.asarray(w, float).reshape(len(up), -1)
H.hci_two_rdm(h, up, dn, w[:, 0])          # warm-up
t0 = time.perf_counter(); D = H.hci_one_rdm(h, up, dn, w[:, 0]); t1 = time.perf_counter()
d2 = H.hci_two_rdm(h, up, dn, w[:, 0]); t2 = time.perf_counter()
G = H.spin_free_two_rdm(d2)
rec = measure(g, h, D, G)
og = g.orbital_gradient(D, G)
U = H.rotation_from_kappa(H.orbital_step(og["gradient"], og["hdiag"], h.orbsym[1:h.norb + 1]))
g.rotate_integrals(U)
rot = []
for _ in range(args.repeats):
    t3 = time.perf_counter(); g.rotate_integrals(U); rot.append(1e3 * (time.perf_counter() - t3))
g.close()
rec.update({"system": "C2_r1.24253 cc-pVDZ, state 1 of the eps_var %g wavefunction (two states, one iteration), %d determinants" % (args.eps_var, len(up)),
            "one_rdm_wall_ms": 1e3 * (t1 - t0), "two_rdm_wall_ms": 1e3 * (t2 - t1), "rotate_integrals_wall_ms_median": med(rot),
            "max_abs_gradient": float(np.max(np.abs(og["gradient"])))})
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
    g = sqmc_amd.GpuChem(n, 1, 1, np.ones(n1, np.int32), prod.reshape(-1), c2.reshape(-1), packed, n_group=1)
    host = H.ChemHost.__new__(H.ChemHost)              # what dense_integrals reads, nothing else
    host.norb, host.combine_2, host.integrals = n, c2, packed
    D = rng.uniform(-1.0, 1.0, (n, n)); D = D + D.T
    G = rng.uniform(-1.0, 1.0, (n,) * 4)
    G = G + G.transpose(2, 3, 0, 1); G = G + G.transpose(1, 0, 3, 2)
    rec = measure(g, host, D, G)
    g.close()
    rec["system"] = "dense random integrals, random symmetric D, G with G[pqrs] = G[rspq] = G[qpsr]"
    records.append(rec)
    print(json.dumps(rec), flush=True)

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    commit = None
doc = {"tool": "tools/orbopt_time.py", "command": "python tools/orbopt_time.py --repeats %d --eps-var %g" % (args.repeats, args.eps_var),
       "commit": commit, "device": torch.cuda.get_device_name(0), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
