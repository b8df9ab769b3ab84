"""The head of a step -- the spawn gate, the child offsets of their five producers, gate_block_parents, k_spawn's parent search,
spawn_emit's slots and flags -- through sqmc_gpu_step and sqmc_gpu_run against the independent model (tests/head_checker.py), at
the seams the cases of tests/head_cases.py are built on (tests/golden/README_step_head.md lists them).

One fresh child per variant, one after the other (the library reads its switches once per process); the first child that fails ends
the test, and nothing more is started on the GPU.  Every child asserts sqmc_gpu_debug_last_head -- a variant that silently ran another
head proves nothing -- and compares, per case: out_stats[15] == the model's children == the spawn slots of debug_premerge (two per
child with the heat-bath proposal); per slot, a model weight of 0 <=> a record weight of 0, otherwise up, dn, wt, imp_distance and
initiator bit for bit.  No tolerance: every quantity is an integer, a flag, or one product of two doubles.  REPLAY's generator must
end where the model's ends.  The tail is not re-tested here."""
import json
import os
import subprocess
import sys
import time

import pytest

import head_cases as HS
import test_head_checker as TH

HERE = os.path.dirname(os.path.abspath(__file__))
# seconds a child may take: the slowest measured on an MI355X took 1.2 s, start-up and the oracle's build check included
# (README_step_head.md has every child's time); the limit leaves room for a cold file cache and a busy host
CHILD_LIMIT = 60


@pytest.fixture(scope="module")
def case_files(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("head_seams")
    t0 = time.time()
    cases, _, _ = TH.built(oracle)
    files = dict(first=str(d / "first.pkl"), p=str(d / "p.pkl"))
    HS.write(files["first"], cases)
    HS.write(files["p"], HS.build_p())
    print("cases and the model's answers: %.1f s on the CPU" % (time.time() - t0))
    return files, cases


def _child(path, variant):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_")}
    env.update(HS.VARIANTS[variant][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "head_cases.py"), path, variant], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
    wall = round(time.time() - t0, 2)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(json.dumps(x) for x in recs))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (variant, r.returncode, bad[:5], r.stdout[-1500:], r.stderr[-1500:])      # the first child that fails ends the test
    print("variant %s: child took %.2f s" % (variant, wall))
    return [x for x in recs if "case" in x], wall


@pytest.mark.gpu
def test_first_step_heads(case_files):
    """sets G, W, S and H on a first step: k_gate + scan + k_spawn's narrowing (COUNTER), k_replay_prepass + k_spawn (REPLAY: G and W)"""
    files, cases = case_files
    walls = {}
    for variant in ("first_counter", "first_replay"):
        recs, walls[variant] = _child(files["first"], variant)
        mode = HS.VARIANTS[variant][1]
        assert [x["case"] for x in recs] == [c["name"] for c in cases if mode in c["want"] and HS.runs_in(c, HS.VARIANTS[variant][2])]
        assert all(x["status"] == (1 if "short_of_mwalk" in x["case"] else 0) for x in recs)
    print("child wall times:", json.dumps(walls))


@pytest.mark.gpu
def test_pipelined_second_step_per_offsets_producer(case_files):
    """set P: the second step of a pipelined run, once per producer of the child offsets; the heat-bath and the unpacked electron-gas
    lists ride on the radix variant"""
    files, _ = case_files
    walls, heads = {}, {}
    for variant in [v for v in HS.VARIANTS if v.startswith("p_")]:
        recs, walls[variant] = _child(files["p"], variant)
        assert len(recs) == (3 if HS.VARIANTS[variant][2] == "P+H" else 1), recs
        heads[variant] = {x["case"]: x["head"] for x in recs}
    print("heads:", json.dumps(heads))
    print("child wall times:", json.dumps(walls))
