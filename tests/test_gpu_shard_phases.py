"""The sharded (multi-rank) step phase by phase against an independent model (tests/shard_checker.py; the finish:
tests/anneal_checker.py).  sqmc_gpu_shard_begin / _pack / _finish take device pointers and communicate nothing, so ONE process
drives R ranks' worth of contexts and does the exchanges in numpy: no gloo, no RCCL, no process group.

The GPU work runs in fresh children (tests/shard_phase_cases.py), one after the other: torch has to be imported before the HIP
library, and the library reads SQMC_SHARD_BUCKET / SQMC_BUCKET_HOLDOFF once per process.  A child prints one JSON line per
check and its wall time; the first child that fails ends its test, and nothing more is started by it.

Tolerances.  Every comparison is bit for bit (dyadic inputs: the projection at row-length seams, the routing as 64-bit words, the
finish on records built by hand) or within a bound derived from proposal_checker.rounding_bound in the docstring of the case
(run_physics, finish_compare, run_natural in shard_phase_cases.py); none is fitted to what the library returns, and no case
leaves a walker or a determinant out of its comparison.

What the cases hold to the model: k_prj_gather_rows (x_global, zeros included), k_prj_apply_rows and k_prj_apply at full row
lengths 1, 2, 63, 64, 65, 127, 128, 129 and 193 (one rank: sqmc_gpu_step and sqmc_gpu_run of two steps, plain and chained; R = 2
and 3 by hash, every rank; R = 3 by hand with a rank that owns no row and a rank that owns the rows of 64 and 128), death/clone
and H_ii against the second-quantised H, the host-built projector against -tau H_ij, k_child_owner + the stable 8-bit sort +
k_pack_send for ranks (1, 2), (2, 3), (100, 255) under both owner hashes on C2 (uniform), the 57-plane-wave electron gas
(two-array keys) and the 10-electron C2 (heat-bath, two slots per child), k_unpack_recv and the n0 / n_recv bookkeeping of
sqmc_gpu_shard_finish on the radix and on the bucket tail, and the composition of all of it at R = 2 and 3.

Which route the second step of sqmc_gpu_run takes: the pipelined head pre-computes y = A x (d_prj_y, k_prj_finish_rows' closing
line in the step) only behind a bucket tail; the library has no door that says whether it did.  The projection child
therefore runs twice, on the default (bucket) tail and with SQMC_BUCKET=0 on the radix tail, where k_prj_apply is a kernel of
its own, and reports sqmc_gpu_last_tail and the count of bucket steps of every run; the tail is asserted, the route behind it
is not, and the bits must be the model's either way."""
import json
import multiprocessing
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import proposal_checker as PC
import shard_phase_cases as CASES
from conftest import FCIDUMP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(mode, outdir, at_least):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SQMC_")}
    env.update(CASES.ENV[mode])
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "shard_phase_cases.py"), mode, str(outdir)], env=env, capture_output=True, text=True, timeout=300)
    wall = time.time() - t0
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(json.dumps(x) for x in recs))
    print("child %s: wall time %.2f s" % (mode, wall))
    bad = [x for x in recs if x.get("ok") is False]
    assert r.returncode == 0 and not bad, (mode, bad[:5], r.stdout[-1500:], r.stderr[-2500:])
    cases = [x for x in recs if "case" in x]
    assert len(cases) >= at_least, (mode, len(cases))
    return {x["case"]: x for x in cases}


@pytest.mark.parametrize("mode", ["projection", "projection_radix"])
def test_projection_at_row_length_seams_bit_for_bit(tmp_path, mode):
    """shard_phase_cases.run_projection: its docstring states why no child of a deterministic parent touches a deterministic
    weight (spawn_emit marks it imp_distance -1, the merge does not add it: do_walk.f90:5950) and why min_wt = 2^200."""
    got = run_child(mode, tmp_path, 3 + 2 * 2 + 3 * 3 + 3 + 1)
    seen = set()
    for tag, R in (("hash_R2", 2), ("hash_R3", 3), ("hand_R3", 3)):
        for r in range(R):
            seen |= set(got["%s_rank%d_pack" % (tag, r)]["lengths"])
        assert seen >= set(CASES.SC.SEAM_LENGTHS), (tag, sorted(seen))        # every seam length was some rank's row
        seen = set()
    assert got["hand_R3_rank2_begin"]["rows"] == 0 and got["hand_R3_rank2_begin"]["walkers"] == 40
    assert {64, 128} <= set(got["hand_R3_rank1_pack"]["lengths"])
    assert got["one_rank_step"]["children"] > 0
    for k in ("one_rank_run2_plain", "one_rank_run2_chained"):
        print("%s: last tail %r, bucket steps %d" % (k, got[k]["last_tail"], got[k]["bucket_steps"]))
        assert (got[k]["last_tail"]["kind"], got[k]["bucket_steps"]) == (("radix", 0) if mode == "projection_radix" else ("bucket", 2))


def test_death_clone_and_the_real_projector_against_the_independent_h(tmp_path):
    """R = 3, the real population and projector (shard_phase_cases.run_physics derives the tolerances).  The projector itself, here
    on the CPU: every stored s.prj_values entry is -tau H_ij of proposal_checker.ChemH within tau * rounding_bound(terms of
    H_ij) -- the one rounding of the product with tau is inside that bound (4 n 2^-53 sum |terms| >= 2^-53 |H_ij|)."""
    got = run_child("physics", tmp_path, 6)
    n_all = 0
    for r in range(3):
        c = got["physics_rank%d_pack" % r]
        assert c["compared"] == c["walkers"] and c["stochastic"] > 300 and c["deterministic"] > 200
        n_all += c["walkers"]
    assert n_all > 2400
    with np.load(os.path.join(str(tmp_path), "projector.npz")) as z:
        counts, indices, values, iu, idn, tau, order = (z[k].copy() for k in ("counts", "indices", "values", "imp_up", "imp_dn", "tau", "orb_order"))
    rows_of = np.repeat(np.arange(len(counts)), counts)
    nnz, nproc = len(values), 4
    cuts = [nnz * q // nproc for q in range(nproc + 1)]
    jobs = [(FCIDUMP, order, float(tau), rows_of, indices, values, iu, idn, cuts[q], cuts[q + 1]) for q in range(nproc)]
    t0 = time.time()
    with multiprocessing.get_context("spawn").Pool(nproc) as pool:       # CPU only: the workers import numpy and the checkers, nothing of the GPU
        res = pool.map(CASES.SC.projector_against_h, jobs)
    assert all(bad is None for _, bad, _ in res), [bad for _, bad, _ in res if bad is not None][:3]
    assert sum(n for n, _, _ in res) == nnz > 10000
    print("projector: %d stored entries in %.1f s, largest |difference| / bound = %.3g" % (nnz, time.time() - t0, max(w for _, _, w in res)))


@pytest.mark.parametrize("system", ["c2", "heg57", "heatbath"])
def test_routing_for_ranks_other_than_zero(tmp_path, system):
    """The records of the (0, 1) twin -- same walker list, raw seed and step number, hence the same children -- passed through
    shard_checker.route with owners from an independent source equal the send buffer of (r, R) as 64-bit words, counts
    included; rows behind sum(counts) keep their -1 fill; at R = 255 at least 200 destinations stay empty; at R = 3 no
    destination gets less than a fifth.  c2 also holds the refusals of sqmc_gpu_shard_config / _begin (the refused context
    then serves as a twin and must pack what a fresh one packs)."""
    got = run_child("routing_" + system, tmp_path, 2 + 6 + (1 if system != "c2" else 10))
    tag = system
    for (r, R) in ((1, 2), (2, 3), (100, 255)):
        for h in (0, 1):
            c = got["%s_r%d_R%d_hash%d" % (tag, r, R, h)]
            assert c["records"] > (1000 if R < 255 else 0) and c["children"] > 0
            if R == 255:
                assert c["empty_destinations"] >= 200
    if system == "heatbath":
        c = got["heatbath_two_slots_two_destinations"]
        assert c["children_with_both_slots"] >= 1 and min(c["split"].values()) >= 1


@pytest.mark.parametrize("variant", ["radix", "bucket"])
def test_finish_on_received_records_exact_and_rng_free(tmp_path, variant):
    """shard_phase_cases.run_finish / finish_compare: anneal_checker.fold(mid-step residents, records, exact=False) raises no
    NeedsDraw, the list is the model's bits, the sums are anneal_checker.sums: exactly where every weight is dyadic (the
    empty rank), else within rounding_bound(n, sum |terms|) for the order of the additions -- the stochastic residents carry
    the death/clone factor -- and the table sums within rounding_bound of their own terms.  Each child asserts through
    sqmc_gpu_last_tail that it ran the tail it was written for."""
    got = run_child("finish_" + variant, tmp_path, 5)
    assert got["finish_%s_rank0_recv1500" % variant]["tail"]["kind"] == ("bucket" if variant == "bucket" else "radix")
    assert got["finish_%s_rank0_recv1500" % variant]["n_recv"] == 1500 and got["finish_%s_rank0_recv1500" % variant]["n0"] >= 256
    assert got["finish_%s_empty_rank_recv0" % variant]["nwalk"] == 0 and got["finish_%s_empty_rank_recv40" % variant]["n0"] == 0


def test_the_natural_step_conserves_what_it_was_given(tmp_path):
    got = run_child("natural", tmp_path, 2 * 2 + 2 + 3)
    for R in (2, 3):
        assert sum(got["natural_R%d_rank%d_finish" % (R, q)]["n_recv"] for q in range(R)) == sum(got["natural_R%d_every_record_goes_to_its_owner" % R]["sent"]) > 1000
