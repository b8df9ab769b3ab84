"""The step variant hf_to_psit at its seams -- wave_sum_4096 / wave_tree_sum over C(T) and Psi_T, k_psit_apply, k_anneal<2, 1> and
k_anneal<3, 1> with fold_slot<1>, the go.ps_raw copy k_psit_finish sums for T^-1, the p.koff branches of k_gate, k_spawn and
k_spawn_keys -- against the independent model (tests/psit_checker.py) on the cases of tests/psit_cases.py.

One fresh child per variant, one after the other (the library reads its switches once per process): default, SQMC_ANNEAL_ITEMS=3,
SQMC_FORCE_UNPACKED=1, and both.  Every child asserts through sqmc_gpu_last_tail the shape it ran -- the radix tail, two or three
slots per thread, packed or unpacked keys; the two lists of 2^20 - 1 and 2^20 sorted slots assert 2 and 3 slots per thread with no
switch set -- and compares, per case and sum order: set H, the premerge weights with head(), the spawn slots and out_stats[15] with
children(), no weight spawned onto the first determinant, the new list with tail() of the device's own spawn records; set T, the new
list, flags and cached H_ii; all bit for bit.  The 16 sums stay within N 2^-53 sum|term| of their correctly rounded value, N the
number of terms: the longest chain any reduction can have (psit_cases.stat_bound) -- not the 1e-11 of test_gpu_parity._sums_close.
A child that dies or fails ends the test there."""
import json
import os
import subprocess
import sys
import time

import pytest

import psit_cases as PC
import test_psit_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def case_files(c2_walk, tmp_path_factory):
    d = tmp_path_factory.mktemp("psit_seams")
    b = TC.built(c2_walk)
    print("cases and the model's answers: %.1f s on the CPU" % b["seconds"])
    files = {}
    for items in (2, 3):
        files[items] = str(d / ("cases_items%d.pkl" % items))
        PC.write(files[items], b["tables"], b["H"] + b["T"][items], (b["uu"], b["ud"]) if items == 2 else None)
    return files, b


def _child(path, variant, limit):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_")}
    env.update(PC.VARIANTS[variant][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "psit_cases.py"), path, variant], env=env, capture_output=True, text=True, timeout=limit)
    wall = round(time.time() - t0, 2)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(json.dumps(x) for x in recs if "case" in x))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (variant, bad[:5], r.stdout[-1500:], r.stderr[-1500:])      # the first child that fails ends the test: nothing more is started
    return [x for x in recs if "case" in x], wall


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(PC.VARIANTS))
def test_psit_seams(case_files, variant):
    files, b = case_files
    env, items = PC.VARIANTS[variant]
    recs, wall = _child(files[items], variant, 300)
    print("variant %s: child took %.2f s, %d runs" % (variant, wall, len(recs)))
    ran = {(x["case"], x["sum_order"]) for x in recs if "sum_order" in x}
    assert ran == {(c["name"], o) for c in b["H"] + b["T"][items] for o in (0, 1) if PC.runs_in(c, variant, o)}, "every case, in both sum orders, none skipped"
    assert ("refusals_beyond_64^3" in {x["case"] for x in recs}) == (items == 2)
    for x in recs:
        if "tail" in x:
            assert x["tail"]["kind"] == "radix" and x["tail"]["packed"] == ("unpacked" not in variant), x
            big = x["case"].startswith("sorted_slots_")
            assert x["tail"]["items"] == (items if not big else (3 if x["case"].endswith(str(1 << 20)) else 2)), x
    if variant in PC.NO_SWITCH:
        assert {x["case"] for x in recs} >= {"sorted_slots_%d" % n for n in ((1 << 20) - 1, 1 << 20)}
    h = [x for x in recs if x["case"].startswith("H_") and x["n_ct"] > 1]
    assert sum(x["n_out"] for x in h) > 1000 and sum(x["n_discarded"] for x in h) > 100, "the steps spawn outside C(T), and discard there"
    worst = max(max(x["ratio_tinv"].values()) for x in h)
    print("variant %s: largest |T^-1 sum - exact| / (2^-53 sum|term|): %.3g" % (variant, worst))
