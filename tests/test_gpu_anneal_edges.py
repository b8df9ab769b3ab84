"""sqmc_gpu_annihilate at tile seams, at the resident / spawn seam, on degenerate lists, at the bucket tail's capacities and at the
reference's stops, against the independent fold model (tests/anneal_checker.py), once per tail variant.

The library reads which tail it runs from the environment once per process, so the cases (tests/anneal_edge_cases.py) run in
one fresh child per variant, one after the other; each child prints one JSON line per case with the tail sqmc_gpu_last_tail
reported, which must be the one the case was written for.  All cases are exact and RNG-free, so every variant -- the bucket
tail, the radix tail with 2, 3 and 4 slots per thread in both RNG disciplines, the spawn-only sort + merge path, unpacked keys --
must return the model's bits.  Tile size T = 256 x slots per thread: 512, 768, 1024.

The one stochastic part, the rounding of reduce_my_walker, has a case of its own (COUNTER discipline, fixed seed): 3 x 4,096
children at |w| = q min_wt; survivors carry +-min_wt x reweight_factor_inv, nothing else changes, and the survivor count of each
class lies within 5 binomial standard deviations of 4096 q -- confirmed for the oracle's COUNTER stream on the CPU first.

C(T): one case gives the library the walk set-up's table and the model e_num(i) = sum_j H_ij c_j from the second-quantised H of
proposal_checker; with dyadic weights only the table carries rounding, and the bound on each sum is derived from
proposal_checker.rounding_bound of every entry (below)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import anneal_checker as AC
import anneal_edge_cases as EC
import proposal_checker as PC
from conftest import FCIDUMP

HERE = os.path.dirname(os.path.abspath(__file__))


def universe(c2_setup, n=3400):
    """a sorted universe of determinants: every k-th of C(T), and as the last one the largest determinant there is (orbitals
    norb-4 .. norb-1 in both spins).  One in eight, and all of Psi_T, are in the C(T) table the library is given."""
    where = {(int(u), int(d)): i for i, (u, d) in enumerate(zip(c2_setup.ct_up, c2_setup.ct_dn))}
    psi = np.array(sorted(where[(int(u), int(d))] for u, d in zip(c2_setup.psi_up, c2_setup.psi_dn)), np.int64)      # Psi_T: the entries with e_den /= 0
    ix = np.unique(np.concatenate([np.linspace(0, len(c2_setup.ct_up) - 1, n).astype(np.int64), psi]))
    top = np.uint64(0b1111 << 22)
    assert int(c2_setup.ct_up[-1]) < int(top)
    uu = np.concatenate([c2_setup.ct_up[ix], [top]]).astype(np.uint64)
    ud = np.concatenate([c2_setup.ct_dn[ix], [top]]).astype(np.uint64)
    in_table = np.unique(np.concatenate([ix[::8], psi]))
    return uu, ud, in_table


def tables_of(sysm):
    return dict(norb=int(sysm.norb), nup=int(sysm.nup), ndn=int(sysm.ndn), orbsym=sysm.orbsym(), prod=sysm.prod().reshape(-1), combine_2=sysm.combine_2().reshape(-1),
                integrals=sysm.integrals(), n_group=int(sysm.s.n_group))


def ct_case(uu, ud, c2_walk, c2_setup, ct_lib, in_table):
    """C(T) on the device against the independent H.  The library holds the set-up's table (ct_lib), the model the table from
    proposal_checker.ChemH.  Entry i of the two differs by at most b_i = rounding_bound(terms of e_num(i)); e_den(i) = c_i is
    a copy on both sides.  With dyadic weights w_i the products are exact up to one rounding, so, D_i = |w_i| b_i:
      e_num_gen, e_num_abs: sum D_i;   e_num2: sum (2 |e_num_i w_i| D_i + D_i^2);   e_num_e_den: sum |e_den_i w_i| D_i;
      e_den_gen, e_den2, e_den_abs: 0 -- each plus rounding_bound(number of terms, sum |terms|) for the order of the additions."""
    H = PC.ChemH(FCIDUMP, [c2_walk.s.orb_order[i] for i in range(1, c2_walk.norb + 1)])
    dets = [(int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])) for i in in_table]
    ct_h, spread = AC.ct_from_h(H, c2_setup.psi_up, c2_setup.psi_dn, c2_setup.psi_c, dets)
    b = EC.Builder(uu, ud, 4242); b.filler(1800)
    case = b.finish("ct_table_against_independent_H", prm=dict(reweight_factor_inv=0.5))
    m = AC.fold(case["res"], case["sp"], case["prm"])
    st, sp_ = AC.sums(m, case["prm"], ct_h)
    lin = q2 = mix = 0.0
    n_terms = 0
    for u, d, w in zip(m["up"], m["dn"], m["wt"]):
        k = (int(u), int(d))
        if k in ct_h and ct_h[k][0] * w != 0.0:
            D = abs(w) * PC.rounding_bound(*spread[k])
            lin += D; q2 += 2 * abs(ct_h[k][0] * w) * D + D * D; mix += abs(ct_h[k][1] * w) * D
            n_terms += 1
            assert abs(ct_lib[k][0] - ct_h[k][0]) <= PC.rounding_bound(*spread[k]) and ct_lib[k][1] == ct_h[k][1], k
    assert n_terms > 100 and abs(st[3]) > 1.0 and st[12] > 0.1
    extra = {2: 0.0, 3: lin, 9: q2, 10: 0.0, 11: lin, 12: 0.0, 13: mix}
    case["stat_bound"] = {k: extra[k] + PC.rounding_bound(*sp_[k]) for k in extra}
    case["ct_model"] = ct_h
    return case


def counter_draws(oracle, c2_walk):
    """the rounding draw of the oracle's COUNTER stream (stage 2, keyed by the determinant) for the seed of the cases, step 0"""
    L = oracle.lib()
    L.orc_det_rank.restype = C.c_uint64
    L.orc_det_rank.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    L.orc_rng_set_mode.argtypes = [C.c_void_p, C.c_int]
    rng = oracle.Rng()
    L.orc_setrn(C.byref(rng), (C.c_int * 4)(*EC.SEED))
    L.orc_rng_set_mode(C.byref(rng), 1)

    def draw(up, dn):
        L.orc_rng_seek(C.byref(rng), 2, L.orc_det_rank(int(c2_walk.norb), int(c2_walk.ndn), up, dn))
        return L.orc_rannyu(C.byref(rng))
    return draw


def rounding_case(oracle, c2_walk, c2_setup):
    n_ct = len(c2_setup.ct_up)
    pick = np.unique(np.linspace(0, n_ct - 1, 3 * 4096 + 200).astype(np.int64))
    assert len(pick) == 3 * 4096 + 200
    case = EC.rounding_case(c2_setup.ct_up, c2_setup.ct_dn, pick[::62][:200], np.setdiff1d(pick, pick[::62][:200])[:3 * 4096])
    # on the CPU: the oracle's COUNTER stream meets the binomial condition for this seed
    m = AC.fold(case["res"], case["sp"], case["prm"], exact=True, draw=counter_draws(oracle, c2_walk))
    v = EC.rounding_verdict(case, m["up"], m["dn"], m["wt"])
    assert isinstance(v, tuple), v
    assert len(m["rounded"]) == 3 * 4096
    return case


@pytest.fixture(scope="module")
def case_files(oracle, c2_walk, c2_setup, tmp_path_factory):
    d = tmp_path_factory.mktemp("anneal_edges")
    uu, ud, in_table = universe(c2_setup)
    ct_lib = {(int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])): (float(c2_setup.ct_num[i]), float(c2_setup.ct_den[i])) for i in in_table}
    tabs = tables_of(c2_walk)
    files = {}
    for T in (512, 768, 1024):
        extra = [ct_case(uu, ud, c2_walk, c2_setup, ct_lib, in_table), rounding_case(oracle, c2_walk, c2_setup)] if T == 512 else []
        files[T] = str(d / ("cases_T%d.pkl" % T))
        EC.prepare(files[T], tabs, uu, ud, ct_lib, T, extra)
    return files


def test_cases_are_exact_and_hit_their_slots(oracle, c2_walk, c2_setup):
    """CPU: every case passes the precondition (prepare asserts it), and the seam cases sit where they are meant to in the sorted list"""
    uu, ud, in_table = universe(c2_setup)
    for T in (512, 768, 1024):
        cases = {c["name"]: c for c in EC.build_cases(uu, ud, T, EC.bucket_constants())}
        for nall in (T - 1, T, T + 1, 2 * T, 3 * T + 1):
            c = cases["nall_%d" % nall]
            assert len(c["res"]["up"]) + len(c["sp"]["up"]) == nall and len(c["res"]["up"]) >= 64

        def runs(c):
            keys = sorted([(int(u), int(d)) for u, d in zip(c["res"]["up"], c["res"]["dn"])] +
                          [(int(u), int(d)) for u, d, w in zip(c["sp"]["up"], c["sp"]["dn"], c["sp"]["wt"]) if w != 0])
            out, start = [], 0
            for i in range(1, len(keys) + 1):
                if i == len(keys) or keys[i] != keys[start]:
                    out.append((start, i - start)); start = i
            return out
        assert (T - 7, 7) in runs(cases["run_ends_on_slot_T-1"])
        assert (T, 6) in runs(cases["run_starts_on_slot_T"])
        for tag in ("mixed_zero_sum", "one_sign", "mixed_zero_sum_on_deterministic"):
            r = [x for x in runs(cases["run_of_2T+3_" + tag]) if x[1] == 2 * T + 3]
            assert len(r) == 1 and r[0][0] % T not in (0, T - 1) and r[0][0] < T
        assert sum(1 for x in runs(cases["every_run_64_or_65"]) if x[1] in (64, 65)) == 18
        for c in cases.values():
            AC.check_precondition(c["res"], c["sp"], c["prm"])
            if c["name"].startswith("seam_last_resident"):
                last = (int(c["res"]["up"][-1]), int(c["res"]["dn"][-1]))
                assert sum(1 for u, d in zip(c["sp"]["up"], c["sp"]["dn"]) if (int(u), int(d)) == last) >= 4


@pytest.mark.gpu
def test_annihilation_edges_on_every_tail(case_files):
    T_of = {2: 512, 3: 768, 4: 1024}
    walls = {}
    for variant, (env_add, rng_mode, items) in EC.VARIANTS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_")}
        env.update(env_add)
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(HERE, "anneal_edge_cases.py"), case_files[T_of[items]], variant], env=env,
                           capture_output=True, text=True, timeout=180)
        walls[variant] = round(time.time() - t0, 2)
        print("variant %s: child took %.2f s" % (variant, walls[variant]))
        recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        bad = [x for x in recs if x.get("ok") is False]
        print("\n".join(json.dumps(x) for x in recs if "case" in x))
        assert r.returncode == 0 and not bad, (variant, bad[:5], r.stdout[-1500:], r.stderr[-1500:])      # the first child that fails ends the test: nothing more is started
        assert len([x for x in recs if "case" in x]) >= 35
    print("child wall times:", json.dumps(walls))
