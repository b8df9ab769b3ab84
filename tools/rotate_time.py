#!/usr/bin/env python3
"""What rotating the integrals into new orbitals costs on the device.  One JSON line per norb in 26, 48, 64:

  26       the C2 fixture, rotated into the natural orbitals of the small deck's variational wavefunction (eps_var 5e-3, two states);
  48, 64   dense random integrals in the identity pair order, a random orthogonal matrix.

Per line: HIP-event milliseconds of the three kernels (half 1, half 2, the one-body block; SQMC_ROT_TIME), wall milliseconds of the
sqmc_gpu_rotate_integrals call (upload of the matrix, work-buffer allocation, kernels, copy back), and -- the comparison, not the code under
test -- wall milliseconds of the reference's formulation on this machine's host: four float64 np.tensordot passes over the unpacked
norb^4 tensor (BLAS), not counting the unpacking.  The largest difference between the two results is reported with it.
For C2 the line also holds the wall time of the variational stage beside the rotation, and one turn of the natural-orbital loop: HCI at the
same eps_var in the file's orbitals and in the natural orbitals, ndets and E_var of both."""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("SQMC_ROT_TIME", "1")          # read once when the library first runs a rotation: HIP events around its kernels
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402,F401  before the HIP library: one libamdhip64 per process
import sqmc_amd         # noqa: E402
from sqmc_amd import host as H      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--eps-var", type=float, default=5e-3)
args = ap.parse_args()

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
sqmc_amd.set_device(0)
L = sqmc_amd.load_library()
L.sqmc_gpu_debug_rotate_ms.argtypes = [C.c_void_p] * 4
med = lambda v: float(np.median(v))


def kernel_ms(g):
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    L.sqmc_gpu_debug_rotate_ms(g.h, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def unpack(packed, c2, n):
    a = np.asarray(c2, np.int64)[1:n + 1, 1:n + 1]
    x, y = a[:, :, None, None], a[None, None, :, :]
    hi, lo = np.maximum(x, y), np.minimum(x, y)
    return packed[hi * (hi - 1) // 2 + lo]


def measure(g, U, packed, c2, n):
    g.rotate_integrals(U)          # allocator warm-up
    wall, ker, bits = [], [], set()
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = g.rotate_integrals(U)
        wall.append(1e3 * (time.perf_counter() - t0))
        ker.append(kernel_ms(g)); bits.add(out.tobytes())
    T = unpack(packed, c2, n)
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        X = T
        for _axis in range(4):     # each pass contracts the leading index and appends the new one: after four the order is back
            X = np.tensordot(X, U, axes=(0, 0))
        host.append(1e3 * (time.perf_counter() - t0))
    diff = float(np.max(np.abs(unpack(out, c2, n) - X)))
    return {"norb": n, "repeats": args.repeats, "kernel_ms_half1_median": med([k[0] for k in ker]), "kernel_ms_half2_median": med([k[1] for k in ker]),
            "kernel_ms_one_body_median": med([k[2] for k in ker]), "kernel_ms_half1": [k[0] for k in ker], "kernel_ms_half2": [k[1] for k in ker],
            "abi_call_wall_ms": wall, "abi_call_wall_ms_median": med(wall), "same_bits_every_repeat": len(bits) == 1,
            "host_four_tensordot_passes_wall_ms": host, "max_abs_difference_from_host": diff}, out


# ---- C2: the natural-orbital loop once
h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
sched = (2 * args.eps_var, 2 * args.eps_var)


def variational(host):
    g = host.gpu()
    t0 = time.perf_counter()
    g.set_hb_tables(*host.hb_tables(g))
    t1 = time.perf_counter()
    r = H.hci_variational(host, g, args.eps_var, eps_sched=sched, n_states=2)
    t2 = time.perf_counter()
    g.close()
    return r, t1 - t0, t2 - t1


variational(h)                     # warm-up of the allocator and the code objects
(up, dn, w, e, _), hb_s, var_s = variational(h)
rdm = H.hci_one_rdm(h, up, dn, w)
occ, vec = H.natural_orbitals(rdm, h.orbsym[1:h.norb + 1])
g = h.gpu()
line, packed = measure(g, vec, h.integrals, h.combine_2, h.norb)
g.close()
h2 = h.with_integrals(packed)
(up2, dn2, w2, e2, _), hb2_s, var2_s = variational(h2)
line.update({"system": "C2_r1.24253 cc-pVDZ, natural orbitals of the eps_var %g wavefunction (two states averaged)" % args.eps_var,
             "variational_stage_wall_s": var_s, "heat_bath_table_wall_s": hb_s,
             "natural_orbital_loop": {"eps_var": args.eps_var, "file_orbitals": {"ndets": int(len(up)), "e_var": [float(x) for x in e], "variational_stage_wall_s": var_s},
                                      "natural_orbitals": {"ndets": int(len(up2)), "e_var": [float(x) for x in e2], "variational_stage_wall_s": var2_s}}})
print(json.dumps(line), flush=True)

# ---- 48 and 64 orbitals: dense random integrals
for n in (48, 64):
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
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    line, _ = measure(g, U, packed, c2, n)
    g.close()
    line["system"] = "dense random integrals, random orthogonal matrix"
    print(json.dumps(line), flush=True)
