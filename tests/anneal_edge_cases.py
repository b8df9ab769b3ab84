"""Directed inputs for sqmc_gpu_annihilate at the places where a parallel fold over a sorted list goes wrong, the expected
output of each from the independent model (anneal_checker.py), and the program that puts them through the library.

Two halves, because the library reads its choice of tail from the environment once per process:
  prepare(path, ...)   in the test process: builds the cases for a tile of T = 256 x ITEMS slots, folds each with the model, and
                       writes everything a child needs (the chemistry tables included) to one file;
  python anneal_edge_cases.py FILE VARIANT   in a fresh child whose environment selects the tail: runs every case through the
                       library, compares bit for bit (table sums: within their rounding bound), asserts the tail that ran, and
                       prints one JSON line per case.  Exit 0: all cases equal the model; 1: a mismatch; 3: a HIP failure (it stops
                       at once and starts nothing more on the GPU).

Every case is exact and RNG-free (anneal_checker.check_precondition is asserted on each one): weights are multiples of 0.25
with |w| <= 4, min_wt = cutoff = 0.25, reweight_factor_inv is 1 or 0.5.  REPLAY, COUNTER and every tail must give the same bits.
"""
import json
import math
import os
import pickle
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEED = (1346, 5634, 6635, 4361)
MWALK = 8192

# variant -> (environment, rng_mode, slots per thread of the radix tail's kernel)
VARIANTS = {
    "bucket": ({}, 1, 2),
    "radix_counter": ({"SQMC_BUCKET": "0"}, 1, 2),
    "radix_replay": ({"SQMC_BUCKET": "0"}, 0, 2),
    "items3": ({"SQMC_ANNEAL_ITEMS": "3"}, 1, 3),
    "items4": ({"SQMC_ANNEAL_ITEMS": "4"}, 1, 4),
    "merge0": ({"SQMC_MERGE_SORT_MIN": "0"}, 1, 2),
    "unpacked": ({"SQMC_FORCE_UNPACKED": "1"}, 1, 2),
}


def bucket_constants():
    """BK_T, BK_CAP_S, BK_TARGET of the default (one block per CU) bucket shape, read from the kernel's own header"""
    txt = open(os.path.join(ROOT, "sqmc_amd", "csrc", "bucket_partition.h")).read()
    full = txt.split("#else", 1)[1]
    g = lambda name, t: int(re.search(r"#define %s (\d+)" % name, t).group(1))
    return dict(BK_T=g("BK_T", txt), BK_CAP_S=g("BK_CAP_S", full), BK_TARGET=g("BK_TARGET", full))


# ------------------------------------------------------------------------------------------------ building cases
class Builder:
    """A case is written as its sorted list: records in (determinant, residents first) order.  Determinants come from a sorted
    universe by index, so the slot a record lands on is known when it is written."""

    def __init__(self, univ_up, univ_dn, seed):
        self.uu, self.ud = univ_up, univ_dn
        self.rs = np.random.RandomState(seed)
        self.res, self.sp, self.zeros = [], [], 0
        self.next = 8                      # universe index of the next fresh determinant (the first ones stay free: "smaller than the first resident")

    def slots(self):
        return len(self.res) + len(self.sp)

    def resident(self, wt, imp, init, ps=0, at=None):
        u = self._take(at)
        self.res.append((u, wt, imp, init, ps))
        return u

    def spawn(self, u, wt, imp=2, init=1):
        self.sp.append((u, wt, imp, init))

    def _take(self, at=None):
        if at is None:
            at = self.next
        assert at >= self.next or at < 8, "determinants are handed out in increasing order"
        self.next = max(self.next, at + 1)
        return at

    def fresh(self):
        return self._take()

    def filler(self, n):
        """n slots of ordinary traffic: lone residents of every kind, lone spawns, and short runs"""
        kinds = [(0, 2), (-2, 1), (1, 2), (2, 0), (3, 1), (2, 2), (1, 0)]
        end = self.slots() + n
        i = 0
        while self.slots() < end:
            left = end - self.slots()
            k = i % 5
            if k in (0, 3):
                imp, init = kinds[(i // 5 + k) % len(kinds)]
                u = self.resident(self._w(nonzero=imp >= 1), imp, init)
                if k == 3 and left >= 3:
                    self.spawn(u, self._w(True), int(self.rs.choice([-1, 1, 3])), 1)
                    self.spawn(u, self._w(True), 2, int(self.rs.randint(0, 2)))
            elif k == 1:
                self.spawn(self.fresh(), self._w(True), int(self.rs.choice([1, 2, 5, 127])), 1)
            elif k == 2:
                self.spawn(self.fresh(), self._w(True), 2, 0)          # a non-initiator's child on an empty determinant: discarded
            else:
                u = self.fresh()
                for _ in range(min(left, int(self.rs.randint(2, 5)))):
                    self.spawn(u, self._w(True), int(self.rs.choice([-1, 1, 2])), int(self.rs.randint(0, 2)))
            i += 1
        assert self.slots() == end

    def _w(self, nonzero=False):
        while True:
            w = int(self.rs.randint(-8, 9)) / 4.0
            if w != 0 or not nonzero:
                return w

    def finish(self, name, prm=None, **meta):
        from anneal_checker import default_params
        res = sorted(self.res)
        assert len({r[0] for r in res}) == len(res)
        order = self.rs.permutation(len(self.sp))
        # creation order: a shuffle of the whole list that keeps the order inside every run (the run cases are written in the order they mean)
        by_run = {}
        for k in sorted(order.tolist()):
            by_run.setdefault(self.sp[k][0], []).append(self.sp[k])
        sp = []
        cursor = {u: 0 for u in by_run}
        for k in order.tolist():
            u = self.sp[k][0]
            sp.append(by_run[u][cursor[u]]); cursor[u] += 1
        zero_at = sorted(self.rs.randint(0, len(sp) + 1, self.zeros).tolist(), reverse=True)
        for z in zero_at:
            sp.insert(z, (int(self.rs.randint(0, len(self.uu))), 0.0, 2, 1))
        ix = np.array([r[0] for r in res], np.int64)
        sx = np.array([s[0] for s in sp], np.int64)
        case = dict(name=name, prm=default_params(**(prm or {})), meta=meta,
                    res=dict(up=self.uu[ix], dn=self.ud[ix], wt=np.array([r[1] for r in res], np.float64), imp_distance=np.array([r[2] for r in res], np.int8),
                             initiator=np.array([r[3] for r in res], np.int8), perm_sign=np.array([r[4] for r in res], np.int8)),
                    sp=dict(up=self.uu[sx] if len(sx) else np.zeros(0, np.uint64), dn=self.ud[sx] if len(sx) else np.zeros(0, np.uint64),
                            wt=np.array([s[1] for s in sp], np.float64), imp_distance=np.array([s[2] for s in sp], np.int8),
                            initiator=np.array([s[3] for s in sp], np.int8)))
        return case


def build_cases(uu, ud, T, bk):
    """the cases of one tile size T; bk = bucket_constants().  uu, ud: the sorted universe of determinants (its last one uses
    orbital norb - 1)."""
    cases = []
    seed = [1000 * (T // 256)]

    def B():
        seed[0] += 1
        return Builder(uu, ud, seed[0])

    def run(b, n, weights=None, res=None, imp=2, init=1):
        """a run of n records on one determinant, a resident first if res = (wt, imp, init, ps)"""
        if res is not None:
            u = b.resident(*res); n -= 1
        else:
            u = b.fresh()
        for k in range(n):
            w = weights[k] if weights is not None else b._w(True)
            b.spawn(u, w, imp if not isinstance(imp, (list, tuple)) else imp[k % len(imp)], init if not isinstance(init, (list, tuple)) else init[k % len(init)])
        return u

    # ---- tile seams
    for nall in (T - 1, T, T + 1, 2 * T, 3 * T + 1):
        b = B(); b.filler(nall)
        cases.append(b.finish("nall_%d" % nall, prm=dict(reweight_factor_inv=0.5 if nall % 2 else 1.0)))
    b = B(); b.filler(T - 7); run(b, 7, imp=[2, -1, 3]); assert b.slots() == T; b.filler(40)
    cases.append(b.finish("run_ends_on_slot_T-1"))
    b = B(); b.filler(T); run(b, 6, res=(0.5, 3, 2, 0), imp=[1, 2]); b.filler(33)
    cases.append(b.finish("run_starts_on_slot_T"))
    zero_sum = [0.5, -0.25, -0.25] + [0.25, -0.25] * T
    for tag, wts, res in (("mixed_zero_sum", zero_sum, None), ("one_sign", [0.25] * (2 * T + 3), None),
                          ("mixed_zero_sum_on_deterministic", [0.5] + zero_sum[:-1], (-0.25, 0, 2, 0))):
        b = B(); b.filler(T // 2 + 5); run(b, 2 * T + 3, weights=wts if res is None else wts[1:], res=res, imp=[2, 3, 1], init=[1, 0]); b.filler(T // 3)
        cases.append(b.finish("run_of_2T+3_" + tag, L=2 * T + 3))
    b = B(); b.filler(330)
    for k in range(18):
        run(b, 64 + (k % 2), res=(1.0, 2, 2, 0) if k % 3 == 0 else None, imp=[2, -1, 1, 5], init=[1, 1, 0])
    cases.append(b.finish("every_run_64_or_65"))
    # ---- the resident / spawn seam: the run begins with the LAST resident, everything behind it is a spawn
    for tag, res, imp, wts, prm in (
            ("plain", (1.5, 2, 2, 0), [2, 1, 3], None, {}),
            ("deterministic_resident_sources_minus_one", (0.75, 0, 2, 0), [-1, -1, 2, -1], None, {}),
            ("permanent_initiator", (2.0, 0, 3, 1), [2, 1], [-0.5] * 3 + [-0.25] * 3, {"r_initiator": 1.0}),
            ("permanent_initiator_negative_sign", (-2.0, 1, 3, -1), [2, 1], [0.5] * 3 + [0.25] * 3, {"r_initiator": 2.0}),
            ("permanent_initiator_r_minus_one", (2.0, 1, 3, 1), [2, 1], [-0.5] * 4, {"r_initiator": -1.0})):
        b = B(); b.filler(400)
        n_res = len(b.res)
        run(b, (len(wts) if wts else 9) + 1, weights=wts, res=res, imp=imp, init=[1, 0, 1])
        for _ in range(25):
            b.spawn(b.fresh(), b._w(True), 2, 1)
        cases.append(b.finish("seam_last_resident_" + tag, prm=prm, n_res=n_res + 1))
    # ---- degenerate lists
    b = B(); b.filler(400); b.sp = []
    cases.append(b.finish("no_spawns"))
    b = B(); b.filler(400); b.sp = []; b.zeros = 300
    cases.append(b.finish("all_spawn_weights_zero"))
    b = B(); b.filler(400); b.sp = []; b.spawn(b.res[57][0], 0.75, 3, 1); b.zeros = 40
    cases.append(b.finish("one_nonzero_spawn"))
    b = B(); b.filler(400); b.sp = []
    for (u, w, imp, init, ps) in b.res:
        if imp != 0 and w != 0:
            b.spawn(u, 0.25, 2, 1); b.spawn(u, -w, 3, 0); b.spawn(u, -0.25, -1, 1)
    cases.append(b.finish("spawns_cancel_every_stochastic_resident"))
    b = B(); b.filler(400); b.sp = []
    for k in range(120):
        b.spawn(k % 8, b._w(True), 2, 1)
    cases.append(b.finish("spawns_below_the_first_resident"))
    b = B(); b.filler(400); b.sp = []
    top = len(uu) - 1
    for k in range(120):
        b.spawn(top - 1 - (k % 6), b._w(True), 2, 1)
    cases.append(b.finish("spawns_above_the_last_resident"))
    b = B(); b.filler(400)
    for k in range(9):
        b.spawn(top, 0.5, 2 + k % 2, 1)
    cases.append(b.finish("spawns_on_orbital_norb-1"))
    # ---- the bucket tail's own edges (on every other tail they are ordinary lists)
    for n0 in (63, 64, 65):
        b = B(); b.filler(6 * n0); b.sp = []; b.res = b.res[:n0]
        assert len(b.res) == n0
        for k in range(300):
            b.spawn(b.res[(7 * k) % n0][0] if k % 3 else b.fresh(), b._w(True), int(b.rs.choice([-1, 1, 2])), int(b.rs.randint(0, 2)))
        cases.append(b.finish("residents_%d" % n0))
    for ns in (1, bk["BK_T"] - 1, bk["BK_T"], bk["BK_T"] + 1):
        b = B(); b.filler(500); b.sp = []
        for k in range(ns):
            b.spawn(b.res[(11 * k) % len(b.res)][0] if k % 2 else b.fresh(), b._w(True), int(b.rs.choice([-1, 1, 2])), int(b.rs.randint(0, 2)))
        cases.append(b.finish("spawn_count_%d" % ns))
    for extra in (0, 1):
        # 300 residents in 3 buckets (slots / BK_TARGET): the middle one, residents [100, 200), receives BK_CAP_S (+ 1) spawns
        b = B()
        for k in range(300):
            b.resident(b._w(k % 3 != 0), (0, 2, 1)[k % 3], (2, 1, 0)[k % 3])
            b.fresh()                                # a free determinant behind every resident
        ids = [r[0] for r in b.res]
        mid = ids[100:200]
        for k in range(bk["BK_CAP_S"] + extra):
            r = mid[(13 * k) % 100]
            b.spawn(r + (k % 2), b._w(True), int(b.rs.choice([-1, 1, 2])), int(b.rs.randint(0, 2)))
        for k in range(30):
            b.spawn(ids[(k * 9) % 100] if k % 2 else ids[200 + (k * 3) % 100], b._w(True), 2, 1)
        n_all = 300 + bk["BK_CAP_S"] + extra + 30
        assert (n_all + bk["BK_TARGET"] - 1) // bk["BK_TARGET"] == 3
        cases.append(b.finish("bucket_at_capacity" if not extra else "bucket_over_capacity", retry=bool(extra)))
    b = B()
    for k in range(300):
        b.resident(b._w(k % 3 != 0), (0, 2, 1)[k % 3], (2, 1, 0)[k % 3]); b.fresh()
    ids = [r[0] for r in b.res]
    for k in range(1000):
        b.spawn(ids[(17 * k) % 100] + (k % 2), b._w(True), 2, int(b.rs.randint(0, 2)))      # all below resident 150: the second of the two buckets stays empty
    cases.append(b.finish("empty_bucket"))
    # ---- the reference's stops
    b = B()
    for k in range(100):
        b.resident(b._w(True), 2, 2)
    for k in range(1000):
        b.spawn(b.fresh(), 0.5, 2, 1)
    cases.append(b.finish("merged_list_of_exactly_mwalk", mwalk=1100))
    b = B()
    for k in range(100):
        b.resident(b._w(True), 2, 2)
    for k in range(1001):
        b.spawn(b.fresh(), 0.5, 2, 1)
    cases.append(b.finish("mwalk_plus_one", mwalk=1100, status=1))
    b = B()
    for k in range(150):
        b.resident(b._w(True), 2, 2)
    for (u, w, imp, init, ps) in list(b.res):
        b.spawn(u, -w, 2, 1)
    cases.append(b.finish("total_cancellation_without_deterministic_space", status=4))
    return cases


def expected_tail(variant, case, bk):
    env, rng_mode, items = VARIANTS[variant]
    n0, ns = len(case["res"]["up"]), len(case["sp"]["up"])
    mwalk = case["meta"].get("mwalk", MWALK)
    rows = (ns + bk["BK_T"] - 1) // bk["BK_T"]
    bucket = variant == "bucket" and n0 >= 64 and ns > 0 and rows * bk["BK_T"] <= mwalk
    kind = "radix" if not bucket else ("bucket-retried" if case["meta"].get("retry") else "bucket")
    return dict(kind=kind, items=0 if kind == "bucket" else items, merge=(variant == "merge0" and ns > 0), packed=variant != "unpacked")


def prepare(path, tables, uu, ud, ct, T, extra_cases=()):
    """fold every case with the model and write the file a child reads.  ct: {(up, dn): (e_num, e_den)} of the table the library
    is given; the model's sums use the same numbers here (the table itself is compared with the independent H elsewhere)."""
    import anneal_checker as AC
    bk = bucket_constants()
    cases = build_cases(uu, ud, T, bk) + list(extra_cases)
    for c in cases:
        if c["meta"].get("kind") == "rounding":          # the one case that draws: judged by rounding_verdict, not by equality
            continue
        AC.check_precondition(c["res"], c["sp"], c["prm"])          # fails (not skips) where a draw would be needed
        m = AC.fold(c["res"], c["sp"], c["prm"], exact=True)
        bad = AC.invariants(c["res"], c["sp"], c["prm"], m, m["discarded"], m["reset"])
        assert not bad, (c["name"], bad[:3])
        ctm = c.get("ct_model", ct)
        st, spread = AC.sums(m, c["prm"], ctm, m["n_before"], m["w_abs_before"])
        c["want"] = {k: m[k] for k in ("up", "dn", "wt", "imp_distance", "initiator")}
        c["want_stats"] = st
        c["stat_bound"] = c.get("stat_bound") or {k: 4.0 * spread[k][0] * 2.0 ** -53 * spread[k][1] for k in spread}      # proposal_checker.rounding_bound
        c["n_discarded"], c["n_reset"] = len(m["discarded"]), len(m["reset"])
        c.pop("ct_model", None)
    keys = sorted(ct)
    blob = dict(tables=tables, cases=cases, T=T, bk=bk,
                ct=dict(up=np.array([k[0] for k in keys], np.uint64), dn=np.array([k[1] for k in keys], np.uint64),
                        num=np.array([ct[k][0] for k in keys]), den=np.array([ct[k][1] for k in keys])))
    with open(path, "wb") as f:
        pickle.dump(blob, f)
    return cases


# ------------------------------------------------------------------------------------------------ the child
def _ctx(blob, rng_mode, mwalk, n_imp, ct=None):
    import sqmc_amd
    t = blob["tables"]
    g = sqmc_amd.GpuChem(t["norb"], t["nup"], t["ndn"], t["orbsym"], t["prod"], t["combine_2"], t["integrals"], n_group=t["n_group"],
                         rng_mode=rng_mode, seed=SEED, mwalk=mwalk)
    # the door applies no projector: an empty matrix of the deterministic space's size (stored diagonal, all zero)
    g.set_projector(np.ones(n_imp, np.int64), np.arange(1, n_imp + 1, dtype=np.int64), np.zeros(n_imp))
    ct = ct or blob["ct"]
    g.set_ct_table(ct["up"], ct["dn"], ct["num"], ct["den"])
    return g


def _upload(g, res):
    n = len(res["up"])
    big = np.full(n, 1e51)
    g.upload_walkers(dict(res, matrix_elements=big, e_num=big, e_den=big))


def _compare(case, got, out):
    want, ws = case["want"], case["want_stats"]
    if len(got["up"]) != len(want["up"]):
        return "length %d, model %d" % (len(got["up"]), len(want["up"]))
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        if not np.array_equal(got[k], want[k]):
            i = int(np.nonzero(got[k] != want[k])[0][0])
            return "%s differs first at %d: %r, model %r" % (k, i, got[k][i], want[k][i])
    for k in range(16):
        bound = case["stat_bound"].get(k, 0.0)
        if not abs(out[k] - ws[k]) <= bound:
            return "out_stats[%d] = %r, model %r, bound %r" % (k, out[k], ws[k], bound)
    return None


def run_case(blob, variant, case):
    import sqmc_amd
    env, rng_mode, items = VARIANTS[variant]
    res, sp, prm, meta = case["res"], case["sp"], case["prm"], case["meta"]
    n_imp = int((res["imp_distance"] == 0).sum())
    t0 = time.time()
    g = _ctx(blob, rng_mode, meta.get("mwalk", MWALK), n_imp, case.get("ct"))
    rec = dict(case=case["name"], variant=variant, n0=len(res["up"]), n_spawn=len(sp["up"]))
    try:
        _upload(g, res)
        retries0 = g.tail_stats()[1]
        status, out = 0, None
        try:
            out = g.annihilate(prm, sp)
        except sqmc_amd.SqmcGpuError as e:
            status = e.code
        rec["status"] = status
        if status < 0:
            rec["ok"] = False; rec["why"] = "library failure"
            return rec
        want_status = meta.get("status", 0)
        why = None if status == want_status else "status %d, expected %d" % (status, want_status)
        if status != 1:                      # status 1 is refused at the door, in front of any tail
            tail = g.last_tail(); rec["tail"] = tail
            want_tail = expected_tail(variant, case, blob["bk"])
            if tail != want_tail:
                why = why or "tail %r, this case is written for %r" % (tail, want_tail)
            if g.tail_stats()[1] - retries0 != (1 if want_tail["kind"] == "bucket-retried" else 0):
                why = why or "bucket_retries moved by %d" % (g.tail_stats()[1] - retries0)
        if status == 0 and why is None:
            why = _compare(case, g.download_walkers(), out)
        if want_status != 0 and why is None:
            # nothing was written out of range and the context still works: the same residents with a tame spawn list
            import anneal_checker as AC
            _upload(g, res)
            k = min(50, len(sp["up"]))
            sp2 = {a: v[:k].copy() for a, v in sp.items()}
            sp2["wt"] = np.abs(sp2["wt"]) * np.sign(res["wt"][0])      # nothing cancels
            sp2["up"][:] = res["up"][0]; sp2["dn"][:] = res["dn"][0]
            m = AC.fold(res, sp2, prm, exact=True)
            out2 = g.annihilate(prm, sp2)
            got2 = g.download_walkers()
            for a in ("up", "dn", "wt", "imp_distance", "initiator"):
                if not np.array_equal(got2[a], m[a]):
                    why = "the call after status %d: %s differs from the model" % (status, a)
            if int(out2[5]) != len(m["up"]):
                why = why or "the call after status %d: nwalk" % status
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def main(argv):
    path, variant = argv[1], argv[2]
    for k, v in VARIANTS[variant][0].items():
        assert os.environ.get(k) == v, "the environment of this process does not select variant %s" % variant
    with open(path, "rb") as f:
        blob = pickle.load(f)
    import sqmc_amd
    sqmc_amd.set_device(0)
    t0 = time.time()
    n_bad = 0
    for case in blob["cases"]:
        if case["meta"].get("only") and variant not in case["meta"]["only"]:
            continue
        if case["meta"].get("kind") == "rounding":
            rec = run_rounding(blob, variant, case)
        else:
            rec = run_case(blob, variant, case)
        print(json.dumps(rec, default=str), flush=True)
        if rec.get("status", 0) < 0:
            return 3
        n_bad += 0 if rec["ok"] else 1
    print(json.dumps(dict(variant=variant, cases_failed=n_bad, seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if n_bad else 0


# ------------------------------------------------------------------------------------------------ rounding: the one stochastic case
def rounding_case(uu, ud, res_ix, child_ix):
    """3 x 4096 distinct non-resident determinants, an initiator's children, |w| = q min_wt for q = 1/8, 1/2, 7/8, half of each
    class positive and half negative; COUNTER discipline"""
    from anneal_checker import default_params
    assert len(child_ix) == 3 * 4096
    rs = np.random.RandomState(77)
    n0 = len(res_ix)
    res = dict(up=uu[res_ix], dn=ud[res_ix], wt=rs.randint(1, 9, n0) / 4.0 * rs.choice([-1.0, 1.0], n0), imp_distance=np.where(np.arange(n0) % 4 == 0, 0, 2).astype(np.int8),
               initiator=np.full(n0, 2, np.int8), perm_sign=np.zeros(n0, np.int8))
    q = np.repeat([0.125, 0.5, 0.875], 4096)
    sign = np.tile([1.0, -1.0], 3 * 2048)
    order = rs.permutation(3 * 4096)
    sp = dict(up=uu[child_ix][order], dn=ud[child_ix][order], wt=(q * sign * 0.25)[order], imp_distance=np.full(3 * 4096, 3, np.int8), initiator=np.ones(3 * 4096, np.int8))
    return dict(name="rounding_3x4096", prm=default_params(reweight_factor_inv=0.5), meta=dict(kind="rounding", only=("bucket", "radix_counter"), mwalk=16384),
                res=res, sp=sp, q=q[order])


def rounding_verdict(case, up, dn, wt):
    """the conditions of the rounding case on an output list: every survivor carries +-min_wt x reweight_factor_inv with its own
    sign, no other determinant changed, the survivors per class lie within 5 standard deviations of 4096 q.  None: all hold."""
    prm, res, sp = case["prm"], case["res"], case["sp"]
    unit = prm["min_wt"] * prm["reweight_factor_inv"]
    have = {(int(u), int(d)): float(w) for u, d, w in zip(up, dn, wt)}
    for u, d, w in zip(res["up"], res["dn"], res["wt"]):
        if have.pop((int(u), int(d)), None) != float(w) * prm["reweight_factor_inv"]:
            return "resident (%d, %d) changed" % (u, d)
    counts = {0.125: 0, 0.5: 0, 0.875: 0}
    for u, d, w, q in zip(sp["up"], sp["dn"], sp["wt"], case["q"]):
        g = have.pop((int(u), int(d)), None)
        if g is None:
            continue
        if g != math.copysign(unit, w):
            return "survivor (%d, %d): %r, expected %r" % (u, d, g, math.copysign(unit, w))
        counts[float(q)] += 1
    if have:
        return "%d determinants nobody spawned" % len(have)
    for q, n in counts.items():
        if abs(n - 4096 * q) > 5.0 * math.sqrt(4096 * q * (1 - q)):
            return "class q = %g: %d survivors, binomial mean %g, sigma %.1f" % (q, n, 4096 * q, math.sqrt(4096 * q * (1 - q)))
    return None, counts


def run_rounding(blob, variant, case):
    env, rng_mode, items = VARIANTS[variant]
    res, sp = case["res"], case["sp"]
    t0 = time.time()
    g = _ctx(blob, rng_mode, case["meta"]["mwalk"], int((res["imp_distance"] == 0).sum()))
    rec = dict(case=case["name"], variant=variant, n0=len(res["up"]), n_spawn=len(sp["up"]))
    try:
        _upload(g, res)
        out = g.annihilate(case["prm"], sp)
        got = g.download_walkers()
        rec["tail"] = g.last_tail()
        v = rounding_verdict(case, got["up"], got["dn"], got["wt"])
        rec["ok"] = isinstance(v, tuple) and int(out[5]) == len(got["up"]) and bool(np.all(np.diff(got["up"].astype(np.float64) * 2.0 ** 26 + got["dn"]) > 0))
        rec["status"] = 0
        if isinstance(v, tuple):
            rec["survivors"] = {str(k): n for k, n in v[1].items()}
        else:
            rec["why"] = v
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


if __name__ == "__main__":
    sys.exit(main(sys.argv))
