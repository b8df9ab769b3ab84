"""The sort of k_anneal_bucket's short lists -- one counter per gap, places inside a gap in whatever order the atomics hand them
out, then the rank by (key, slot) -- at its edges, and the radix sort that lists with more residents than it takes still get:
tests/gap_sort_cases.py.  The cases go through sqmc_gpu_annihilate in a child process (bucket_rounds_cases.py's) and are compared
with the independent fold model (tests/anneal_checker.py) under anneal_edge_cases.run_case's criteria: walkers, flags and weights
bit for bit, sums within their rounding bounds, and the tail that ran.  tests/test_gap_sort_cases.py asserts on the CPU that every
case holds what it is named for."""
import json
import os
import subprocess
import sys
import time

import pytest

import anneal_edge_cases as EC
import gap_sort_cases as GS

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def prepared(oracle, c2_walk, c2_setup, tmp_path_factory):
    return GS.prepared(c2_walk, c2_setup, tmp_path_factory)


@pytest.mark.gpu
def test_gap_sort_against_the_fold_model(prepared):
    for c in prepared["cases"]:
        GS.check_case(c, prepared["kc"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_") or k == "SQMC_EXTRA_CFLAGS"}
    env.update(EC.VARIANTS["bucket"][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "bucket_rounds_cases.py"), prepared["path"], "bucket"], env=env, capture_output=True, text=True, timeout=180)
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("child took %.2f s" % (time.time() - t0))
    print("\n".join(json.dumps(x) for x in recs))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (bad[:5], r.stdout[-1500:], r.stderr[-1500:])
    ran = [x for x in recs if "case" in x]
    assert len(ran) == len(prepared["cases"])
    assert all(x["tail"]["kind"] == "bucket" for x in ran), "every case takes the bucket tail, none is re-run through the radix tail"
