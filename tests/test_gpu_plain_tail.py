"""The tail of a step with semistochastic = f -- k_merge at its 256-slot tile, the joins of join_walker2 in both disciplines
(k_join_gather + k_join_par, and the one-lane k_join), the plain drop rule of k_round, k_compact and its sums -- through
sqmc_gpu_annihilate against the independent model (tests/anneal_checker.py: plain_step), at the seams the cases of
tests/plain_tail_cases.py are built on.

One fresh child per variant, one after the other (the library reads SQMC_FORCE_UNPACKED once per process): the parallel joins,
the serial joins on the same COUNTER draws, REPLAY, unpacked keys.  Every child asserts the radix tail without the spawn-only
merge, compares walkers bit for bit -- the draws come from the generator alone: the oracle's COUNTER stream keyed by the later
walker's index among the merged heads, or a 48-bit rannyu in join order, after which the context's generator must stand where the
model's stands -- and checks the draw-free chain layer.  Case C (who carries a chain's weight) runs on the two packed COUNTER
variants, case D (more than JP_CW x JP_TILE sorted slots) alone in a child of its own."""
import json
import os
import subprocess
import sys
import time

import pytest

import plain_tail_cases as PT
import test_plain_tail_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def case_files(oracle, c2_walk, c2_setup, tmp_path_factory):
    d = tmp_path_factory.mktemp("plain_tail")
    base = TC.built(oracle, c2_walk, c2_setup, "base")
    t0 = time.time()
    sets = {k: TC.built(oracle, c2_walk, c2_setup, k) for k in ("A", "B", "C", "D")}
    print("cases and the model's answers: %.1f s on the CPU" % (time.time() - t0))
    files = dict(abc=str(d / "cases_abc.pkl"), d=str(d / "cases_d.pkl"))
    PT.write(files["abc"], base["tables"], sets["A"] + sets["B"] + sets["C"], base["ct"])
    PT.write(files["d"], base["tables"], sets["D"], base["ct"])
    return files, {k: [c["name"] for c in v] for k, v in sets.items()}


def _child(path, variant, limit):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_")}
    env.update(PT.VARIANTS[variant][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "plain_tail_cases.py"), path, variant], env=env, capture_output=True, text=True, timeout=limit)
    wall = round(time.time() - t0, 2)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(json.dumps(x) for x in recs if "case" in x))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (variant, bad[:5], r.stdout[-1500:], r.stderr[-1500:])      # the first child that fails ends the test: nothing more is started
    return [x for x in recs if "case" in x], wall


@pytest.mark.gpu
def test_plain_tail_on_every_variant(case_files):
    files, names = case_files
    walls, carriers = {}, {}
    for variant in PT.VARIANTS:
        recs, walls[variant] = _child(files["abc"], variant, 240)
        print("variant %s: child took %.2f s" % (variant, walls[variant]))
        ran = {x["case"] for x in recs}
        assert len(ran & set(names["A"])) >= 35 and set(names["B"]) <= ran
        assert (set(names["C"]) <= ran) == (variant in PT.C_VARIANTS)
        for x in recs:
            if x.get("status") != 1:
                assert x["tail"]["kind"] == "radix" and x["tail"]["merge"] is False, x
            if x["case"] in names["C"]:
                carriers[variant] = x["carriers"]
    assert set(carriers) == set(PT.C_VARIANTS)
    print("case C, carriers per class (1, 2, 3, 3)/9 of 4096:", json.dumps(carriers), "bounds", [(round(a, 1), round(b, 1)) for a, b in PT.carrier_bounds()])
    print("child wall times:", json.dumps(walls))


@pytest.mark.gpu
def test_window_of_chunk_counts_reloaded(case_files):
    files, names = case_files
    recs, wall = _child(files["d"], "plain_counter", 240)
    print("case D: child took %.2f s" % wall)
    assert [x["case"] for x in recs] == names["D"] and recs[0]["tail"]["kind"] == "radix" and recs[0]["tail"]["merge"] is False
    assert recs[0]["n0"] + recs[0]["n_spawn"] > PT.kernel_constants()["JP_CW"] * PT.kernel_constants()["JP_TILE"]
