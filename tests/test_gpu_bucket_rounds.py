"""k_anneal_bucket at the strides of its phases: buckets whose residents, spawns, merged slots and kept walkers sit one below, on
and one above the block size A = BK_AT (the fold, the rank scan: also 2 A; the compaction, which runs over KEPT walkers in rounds of
CB x A: also CB A), a long run that crosses a round of the fold, every branch of the in-tail H_ii passes, and the
deterministic-space rows of two neighbouring buckets.

Cases and child: tests/bucket_rounds_cases.py.  They go through sqmc_gpu_annihilate with anneal_edge_cases.prepare / run_case and
are compared with the independent fold model (tests/anneal_checker.py): walker lists, weights and flags bit for bit, sums within
the bounds run_case applies; once on the bucket tail and once on the radix tail (COUNTER discipline).  The rows of the
deterministic space are visible through the list (its order, imp_distance 0 where the model has it) and through w_abs_gen_imp.
H_ii of the determinants a bucket creates is compared with the diagonal of proposal_checker.ChemH within rounding_bound of its terms.

Before anything runs on the GPU, every case's targeted bucket is shown to hold exactly the R, S, T and K it is named for -- from
the equal-residents boundary rule b n0 / B, B = ceil(n_all / BK_TARGET), and the model's output (bucket_rounds_cases.layout)."""
import json
import os
import subprocess
import sys
import time

import pytest

import anneal_edge_cases as EC
import bucket_rounds_cases as BR
import proposal_checker as PC
from conftest import FCIDUMP
from test_gpu_anneal_edges import tables_of, universe

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def prepared(oracle, c2_walk, c2_setup, tmp_path_factory):
    """the cases, folded by the model once (prepare), the file the children read, and the layout of every case"""
    kc = BR.kernel_constants()
    uu, ud, in_table = universe(c2_setup, n=max(3400, 5 * kc["A"] + 1500))
    ct_lib = {(int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])): (float(c2_setup.ct_num[i]), float(c2_setup.ct_den[i])) for i in in_table}
    extra = BR.build_cases(uu, ud, kc)
    path = str(tmp_path_factory.mktemp("bucket_rounds") / "cases.pkl")
    cases = [c for c in EC.prepare(path, tables_of(c2_walk), uu, ud, ct_lib, 512, extra) if c["meta"].get("rounds")]
    lays = {c["name"]: BR.check_layout(c, kc) for c in cases}
    # H_ii of the targeted bucket's new determinants from the independent H
    H = PC.ChemH(FCIDUMP, [c2_walk.s.orb_order[i] for i in range(1, c2_walk.norb + 1)])
    for c in cases:
        if "n_hii" in c["meta"]:
            _, of = BR.layout(c, c["want"], kc["BK_TARGET"])
            c["want_me"] = {}
            for i, (u, d, imp) in enumerate(zip(c["want"]["up"], c["want"]["dn"], c["want"]["imp_distance"])):
                if imp >= 1 and of((int(u), int(d))) == c["meta"]["target"]:
                    val, n, sa = H.element(int(u), int(d), int(u), int(d))
                    c["want_me"][i] = (val, PC.rounding_bound(n, sa))
            assert len(c["want_me"]) == c["meta"]["n_hii"]
    # the file again, with want_me in it
    import pickle
    with open(path, "rb") as f:
        blob = pickle.load(f)
    by_name = {c["name"]: c for c in cases}
    for c in blob["cases"]:
        if c["name"] in by_name and "want_me" in by_name[c["name"]]:
            c["want_me"] = by_name[c["name"]]["want_me"]
    with open(path, "wb") as f:
        pickle.dump(blob, f)
    return dict(kc=kc, path=path, cases=cases, lays=lays, nup=int(c2_walk.nup), ndn=int(c2_walk.ndn))


def test_every_case_sits_on_its_stride(prepared):
    """CPU: the targeted bucket of every case holds what the case is named for (check_layout asserts it), and the set is complete"""
    kc, lays = prepared["kc"], prepared["lays"]
    A, CB = kc["A"], kc["CB"]
    t = {name: lay[1] for name, lay in lays.items()}
    for R in (A - 1, A, A + 1):
        assert t["R_%d" % R]["R"] == R and 0 < t["R_%d" % R]["S"] < 16
    for S in (A - 1, A, A + 1):
        assert t["S_%d" % S]["S"] == S and t["S_%d" % S]["R"] < A // 2
    for T in (A - 1, A, A + 1, 2 * A - 1, 2 * A, 2 * A + 1):
        assert t["T_%d" % T]["T"] == T
    T = CB * A + 1
    assert T > 2 * A
    for K in (0, 1, A - 1, A, A + 1, CB * A - 1, CB * A, CB * A + 1):
        o = t["K_%d_of_T_%d" % (K, T)]
        assert o["K"] == K and o["T"] == T
    assert t["K_%d_of_T_%d" % (T, T)]["K"] == T          # K = T: every merged slot is kept
    # the in-tail H_ii passes: which branch each n takes follows from the header's constants (hii_branch); the cases the issue names
    # are there, and between them the cases reach every branch a system of this size (hg = 8) has: 32, 16 and 8 lanes per determinant
    hii = {int(name.split("_")[1]): lay[1] for name, lay in lays.items() if name.startswith("hii_")}
    assert {A // 32, A // 32 + 1, A // 16, A // 16 + 1} <= set(hii)
    lanes = {}
    for n, o in hii.items():
        assert o["K_stoch"] == n
        hg, lanes[n] = BR.hii_branch(n, kc, prepared["nup"], prepared["ndn"])
        assert hg == 8, "C2's 48 terms fit the 8-lane form's room"
    g32, g16 = min(A, kc["HG_GROUPS_CAP"]) // 32, min(A, kc["HG_GROUPS_CAP"]) // 16
    assert lanes[g32] == 32 and lanes[g32 + 1] == 16 and lanes[g16] == 16 and lanes[g16 + 1] == 8 and set(lanes.values()) == {32, 16, 8}
    print("H_ii lanes per determinant by queued determinants:", json.dumps(lanes, sort_keys=True))
    assert "long_run_across_rounds" in t and "deterministic_rows" in t
    assert len(prepared["cases"]) == 3 + 3 + 6 + 8 + 1 + len(hii) + 1
    print(json.dumps({name: lay for name, lay in lays.items()}))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["bucket", "radix_counter"])
def test_bucket_rounds_against_the_fold_model(prepared, variant):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_") or k == "SQMC_EXTRA_CFLAGS"}      # (the flags name the library the cases were sized for)
    env.update(EC.VARIANTS[variant][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "bucket_rounds_cases.py"), prepared["path"], variant], env=env, capture_output=True, text=True, timeout=180)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("variant %s: child took %.2f s" % (variant, time.time() - t0))
    print("\n".join(json.dumps(x) for x in recs))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (variant, bad[:5], r.stdout[-1500:], r.stderr[-1500:])
    assert len([x for x in recs if "case" in x]) == len(prepared["cases"])
    if variant == "bucket":
        assert sum(1 for x in recs if "hii_worst_error_over_bound" in x) == sum(1 for c in prepared["cases"] if "n_hii" in c["meta"])
