"""Directed inputs for k_anneal_bucket at the strides its phases run with, and the child that puts them through the library.

The kernel's block has A = BK_AT threads; its strided phases (gap search, counting pass, scatter, fold) take one more round for
every A elements, the rank scan gives every thread ceil(T / A) merged slots, and the compaction takes one more round for every
CB x A KEPT walkers.  Every case here is a list of B >= 3 buckets in which ONE bucket (the middle one, b = 1) holds exactly the
number of residents R, spawns S, merged slots T = R + S or kept walkers K its name says; layout() derives those numbers again from
the equal-residents boundary rule and the model's output, independently of how the case was written, and the tests assert them
on the CPU before anything runs on the GPU.

  python bucket_rounds_cases.py FILE VARIANT    the child (anneal_edge_cases.run_case per case; the tail is read from the environment
                                                once per process).  Exit 0: every case equals the model; 1: a mismatch; 3: a HIP failure.
"""
import bisect
import json
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

import anneal_edge_cases as EC  # noqa: E402


def kernel_constants():
    """A = BK_AT, CB, BK_LONG_RUN and the bucket shape, read from the kernel's own text"""
    csrc = os.path.join(ROOT, "sqmc_amd", "csrc")
    hii = open(os.path.join(csrc, "hii_group.h")).read()
    bkk = open(os.path.join(csrc, "bucket_kernels.h")).read()
    part = open(os.path.join(csrc, "bucket_partition.h")).read().split("#else", 1)[1]
    g = lambda pat, t: int(re.search(pat, t).group(1))
    # the block size the library is built with: the header's default, unless the build's extra flags (which also name the library
    # file, sqmc_amd/_lib.py) set another
    m = re.search(r"-DBK_AT=(\d+)", os.environ.get("SQMC_EXTRA_CFLAGS", ""))
    k = dict(A=int(m.group(1)) if m else g(r"#define BK_AT (\d+)", hii), CB=g(r"constexpr int CB = (\d+);", bkk), LONG_RUN=g(r"#define BK_LONG_RUN (\d+)", bkk),
             CAP_S=g(r"#define BK_CAP_S (\d+)", part), CAP_R=g(r"#define BK_CAP_R (\d+)", part), CAP_T=g(r"#define BK_CAP_T (\d+)", part))
    k.update(HG_TERMS_DIV=g(r"#define BK_HG_TERMS\(HG\) \(BK_CAP_T / \((\d+) / \(HG\)\)\)", hii),
             HG_GROUPS_CAP=g(r"#define BK_HG_GROUPS\(HG\) \(\(BK_AT < (\d+) \? BK_AT : \d+\) / \(HG\)\)", hii), HG_TASKS=g(r"#define BK_HG_TASKS (\d+)", hii))
    k.update(EC.bucket_constants())
    return k


def hii_branch(n, kc, nup, ndn):
    """lanes per determinant of the in-tail H_ii passes for n queued determinants of a chemistry system without time symmetry:
    bk_hii_group_lanes (hii_group.h) and the choice behind BK_HII_PASSES (bucket_kernels.h), restated from the header's constants"""
    terms_room = lambda hg: kc["CAP_T"] // (kc["HG_TERMS_DIV"] // hg)
    groups = lambda hg: min(kc["A"], kc["HG_GROUPS_CAP"]) // hg
    nuu, ndd, nud = nup * (nup - 1) // 2, ndn * (ndn - 1) // 2, nup * ndn
    terms, tasks = (nup + ndn) + (nuu + ndd) + (nuu + nud + ndd), (nup + ndn) + nuu + ndd + nud
    hg = 8 if (terms <= terms_room(8) and tasks <= 8 * 2 * kc["HG_TASKS"]) else (16 if (terms <= terms_room(16) and tasks <= 16 * kc["HG_TASKS"]) else 0)
    if hg and n <= groups(32) and terms <= terms_room(32):
        return hg, 32
    if hg == 8 and n <= groups(16):
        return hg, 16
    return hg, hg


# ------------------------------------------------------------------------------------------------ the independent layout rule
def layout(case, want, bk_target):
    """Per bucket: residents, spawns, kept walkers, kept walkers outside / inside the deterministic space, from the rule the host
    and the kernel share -- B = ceil(n_all / BK_TARGET) buckets, bucket b >= 1 begins at the key of the resident at position
    b n0 / B -- and from the model's output list `want`.  Keys are (up, dn) pairs: the order of the list."""
    res, sp = case["res"], case["sp"]
    n0, ns = len(res["up"]), len(sp["up"])
    assert np.all(sp["wt"] != 0.0), "a spawn of weight zero is no walker: these cases have none"
    B = min(-(-(n0 + ns) // bk_target), n0)
    rkeys = [(int(u), int(d)) for u, d in zip(res["up"], res["dn"])]
    assert rkeys == sorted(rkeys)
    start = [b * n0 // B for b in range(B + 1)]
    first = [rkeys[start[b]] for b in range(1, B)]
    of = lambda key: bisect.bisect_right(first, key)
    out = [dict(R=start[b + 1] - start[b], S=0, K=0, K_stoch=0, K_det=0) for b in range(B)]
    for u, d in zip(sp["up"], sp["dn"]):
        out[of((int(u), int(d)))]["S"] += 1
    for u, d, imp in zip(want["up"], want["dn"], want["imp_distance"]):
        o = out[of((int(u), int(d)))]
        o["K"] += 1
        o["K_stoch" if imp >= 1 else "K_det"] += 0 if imp == -2 else 1
    for o in out:
        o["T"] = o["R"] + o["S"]
    return out, of


def head_slot(case, of, key):
    """merged slot, inside its bucket, of the first record of determinant `key`: records of the bucket with a smaller key"""
    b = of(key)
    n = sum(1 for u, d in zip(case["res"]["up"], case["res"]["dn"]) if of((int(u), int(d))) == b and (int(u), int(d)) < key)
    return n + sum(1 for u, d in zip(case["sp"]["up"], case["sp"]["dn"]) if of((int(u), int(d))) == b and (int(u), int(d)) < key)


# ------------------------------------------------------------------------------------------------ writing a case bucket by bucket
RES_KINDS = [(0, 2), (2, 2), (1, 1), (3, 2), (-2, 1), (2, 1)]          # (imp_distance, initiator) of an ordinary resident: none is dropped on its own


class Buckets:
    """B buckets of R residents each (so the boundary b n0 / B is b R), written in key order.  A bucket begins with a resident:
    a free determinant in front of the first resident of bucket b would belong to bucket b - 1."""

    def __init__(self, uu, ud, seed, B, R):
        self.b = EC.Builder(uu, ud, seed)
        self.B, self.R, self.cur, self.nres = B, R, -1, R
        self.ids = [[] for _ in range(B)]          # universe index of every resident, per bucket

    def bucket(self):
        assert self.nres == self.R, "bucket %d holds %d residents, not %d" % (self.cur, self.nres, self.R)
        self.cur += 1; self.nres = 0
        return self.cur

    def res(self, wt=None, imp=None, init=None, spawns=()):
        k = RES_KINDS[len(self.b.res) % len(RES_KINDS)]
        imp, init = (k[0] if imp is None else imp), (k[1] if init is None else init)
        u = self.b.resident(self.b._w(True) if wt is None else wt, imp, init)
        self.ids[self.cur].append(u); self.nres += 1
        for (w, i, n) in spawns:
            self.b.spawn(u, w, i, n)
        return u

    def new(self, spawns):
        assert self.nres > 0 or self.cur == 0, "a bucket begins with a resident"
        u = self.b.fresh()
        for (w, i, n) in spawns:
            self.b.spawn(u, w, i, n)
        return u

    def rest(self):
        """the residents the current bucket still lacks, without spawns"""
        while self.nres < self.R:
            self.res()

    def pad(self, buckets, total):
        """spawns on the residents of `buckets` (written already) until the list has `total` slots"""
        k = 0
        while self.b.slots() < total:
            ids = self.ids[buckets[k % len(buckets)]]
            self.b.spawn(ids[(7 * k) % len(ids)], self.b._w(True), int(self.b.rs.choice([1, 2, 3])), int(self.b.rs.randint(0, 2)))
            k += 1

    def finish(self, name, **meta):
        assert self.cur == self.B - 1 and self.nres == self.R
        return self.b.finish(name, rounds=True, **meta)


def build_cases(uu, ud, kc):
    """the cases of one block size A; kc = kernel_constants()"""
    A, CB, TG = kc["A"], kc["CB"], kc["BK_TARGET"]
    cases = []
    seed = [7000 + A]
    kept_new, dropped_new = (0.75, 2, 1), (0.5, 2, 0)      # an initiator's child on a free determinant stays; a non-initiator's is discarded

    def make(name, n_res, fill, need, **meta):
        """fill(bk) writes the middle bucket's content behind its first resident; need = its slots.  The outer buckets carry ordinary
        residents and as many spawns as it takes for B buckets: n_all in ((B - 1) BK_TARGET, B BK_TARGET]."""
        B = 3
        while B * n_res + need + 2 > B * TG:
            B += 1
        assert n_res <= kc["CAP_R"] and need - n_res <= kc["CAP_S"] and need <= kc["CAP_T"]
        seed[0] += 1
        bk = Buckets(uu, ud, seed[0], B, n_res)
        for b in range(B):
            bk.bucket()
            if b == 1:
                fill(bk)
            bk.rest()
        total = max((B - 1) * TG + 50, bk.b.slots() + 2 * (B - 1))
        assert total <= B * TG
        bk.pad([b for b in range(B) if b != 1], total)
        c = bk.finish(name, target=1, **meta)
        cases.append(c)
        return c

    def few_spawns(bk, n):
        for k in range(n):
            if k % 2:
                bk.res(spawns=[(bk.b._w(True), 2, 1)])
            else:
                bk.res(); bk.new([kept_new])

    # ---- residents: R = A - 1, A, A + 1 with a few spawns
    for R in (A - 1, A, A + 1):
        make("R_%d" % R, R, lambda bk: few_spawns(bk, 6), R + 6, R=R, S=6)
    # ---- spawns: S = A - 1, A, A + 1 beside few residents.  chunk = ceil(S / A) x 64 spawns per wave in the counting pass: at A - 1 the
    #      last wave's chunk is partial (63), at A full, at A + 1 (chunk 128) empty -- waves A/128 + 1 .. A/64 - 1 have none, wave A/128 one
    for S in (A - 1, A, A + 1):
        def fill(bk, S=S):
            for k in range(S):
                m = k % 4
                if m == 0:
                    bk.res(spawns=[(bk.b._w(True), 2, int(k % 8 == 0))])
                elif m == 1:
                    bk.new([kept_new])
                elif m == 2:
                    bk.new([dropped_new])
                else:
                    bk.b.spawn(bk.ids[1][-1], bk.b._w(True), 3, 1)
        R = (A + 3) // 4 + 8
        make("S_%d" % S, R, fill, R + S, R=R, S=S)
    # ---- merged slots: T = R + S at every stride of the fold and of the rank scan
    for T in (A - 1, A, A + 1, 2 * A - 1, 2 * A, 2 * A + 1):
        R = T // 2 - 3
        S = T - R

        def fill(bk, R=R, S=S):
            s = 0
            while s < S:
                if s % 3 == 0 and bk.nres < R:
                    n = min(2, S - s)
                    bk.res(spawns=[(bk.b._w(True), 2, 1)] * n); s += n
                else:
                    bk.new([kept_new if s % 2 else dropped_new]); s += 1
        make("T_%d" % T, R, fill, T, R=R, S=S, T=T)
    # ---- kept walkers: K at every stride of the compaction, at a fixed T = CB A + 1.  A resident outside the deterministic space is
    #      cancelled exactly by one spawn of the opposite weight; a non-initiator's child on a free determinant is discarded.
    T = CB * A + 1
    R = (T - 1) // 2 - 24
    S = T - R
    for K in (0, 1, A - 1, A, A + 1, CB * A - 1, CB * A, CB * A + 1):
        def fill(bk, K=K, R=R, S=S):
            cancel = max(R - K, 0)
            keep_new = max(K - R, 0)
            drop_new = S - cancel - keep_new
            assert drop_new >= 0
            for k in range(R):
                w = (1 + k % 8) / 4.0 * (1 if k % 2 else -1)
                if k < cancel:
                    bk.res(w, 2, 2, spawns=[(-w, 2, 1)])
                else:
                    bk.res()
                if k == 0:
                    for _ in range(drop_new):
                        bk.new([dropped_new])
                for _ in range(keep_new // R + (1 if k < keep_new % R else 0)):
                    bk.new([kept_new])
        make("K_%d_of_T_%d" % (K, T), R, fill, T, R=R, S=S, T=T, K=K)
    # ---- a long run whose head sits in the last lanes of the fold's first round and whose followers sit in the second
    L = kc["LONG_RUN"] + 64 + 8
    wts = [0.5] + [0.25, -0.25] * ((L - 1) // 2) + ([0.25] if (L - 1) % 2 else [])
    R = A // 2 + 20
    run = {}

    def fill_run(bk):
        for k in range(A - 2):                       # slots 0 .. A - 3 (the bucket's first resident is slot 0): the head lands on slot A - 2
            if k % 2 == 0 and bk.nres < R - 4:
                bk.res()
            else:
                bk.new([kept_new])
        run["u"] = bk.new([(wts[k], (2, 3, 1)[k % 3], (1, 0)[k % 2]) for k in range(L)])
        for k in range(40):
            bk.new([kept_new if k % 2 else dropped_new])
    c = make("long_run_across_rounds", R, fill_run, A - 2 + L + 40 + 4, L=L, head_slot=A - 2)
    c["meta"]["run_key"] = (int(uu[run["u"]]), int(ud[run["u"]]))
    # ---- determinants that need H_ii in the tail: n kept walkers outside the deterministic space in one bucket, all others of that
    #      bucket inside it.  The passes take 32 lanes per determinant while one pass holds them all, then 16, then 8 (hii_branch); a
    #      pass holds what the weight array has room for, min(A, 512) / lanes groups -- so beside n = A/32, A/32+1, A/16, A/16+1 the
    #      cases sit on those thresholds themselves.  (C2's 4 + 4 electrons take the 8-lane form; the branch of the 16-lane form,
    #      5 + 5 or 6 + 6 electrons, has no system among this door's fixtures and is not run here.)
    g32, g16 = min(A, kc["HG_GROUPS_CAP"]) // 32, min(A, kc["HG_GROUPS_CAP"]) // 16
    for n in sorted({A // 32, A // 32 + 1, A // 16, A // 16 + 1, g32, g32 + 1, g16, g16 + 1}):
        def fill(bk, n=n):
            for k in range(n):
                bk.new([(0.5 + 0.25 * (k % 5), 2, 1)])
                bk.res(imp=0, init=2, spawns=[(0.25, 2, 1)] if k % 3 == 0 else ())
        R = n + 12
        seed[0] += 1
        B = 3
        bk = Buckets(uu, ud, seed[0], B, R)
        for b in range(B):
            bk.bucket()
            if b == 1:
                bk.res(imp=0, init=2)
                fill(bk)
                while bk.nres < R:
                    bk.res(imp=0, init=2)
            bk.rest()
        total = (B - 1) * TG + 50
        bk.pad([0, 2], total)
        c = bk.finish("hii_%d_new_determinants" % n, target=1, n_hii=n)
        cases.append(c)
    # ---- the deterministic-space rows: several kept walkers of imp_distance 0 in the targeted bucket and in the one behind it
    def fill_det(bk):
        for k in range(40):
            bk.res(imp=0 if k % 4 == 0 else 2, init=2, spawns=[(bk.b._w(True), -1 if k % 8 == 0 else 2, 1)] if k % 2 else ())
            bk.new([kept_new])
    make("deterministic_rows", 60, fill_det, 60 + 20 + 40, det_rows=3)
    return cases


def check_layout(case, kc):
    """the CPU assertion of every case: the targeted bucket holds what the case is named for.  Needs case['want'] (prepare)."""
    lay, of = layout(case, case["want"], kc["BK_TARGET"])
    m = case["meta"]
    t = lay[m["target"]]
    assert len(lay) >= 3 and all(o["R"] >= 1 for o in lay), (case["name"], lay)
    for k in ("R", "S", "T", "K"):
        if k in m:
            assert t[k] == m[k], (case["name"], k, t, m[k])
    assert t["S"] <= kc["CAP_S"] and t["T"] <= kc["CAP_T"] and t["R"] <= kc["CAP_R"]
    if m.get("K") == 0:
        assert lay[m["target"] - 1]["K"] > 0 and lay[m["target"] + 1]["K"] > 0, "the empty bucket sits between two that are not"
    if "head_slot" in m:
        A = kc["A"]
        key = m["run_key"]
        assert of(key) == m["target"] and head_slot(case, of, key) == m["head_slot"]
        assert m["head_slot"] % A >= A - 64 and m["head_slot"] % A + m["L"] > A + 64, "head in the last wave of a round, followers through the next"
        assert sum(1 for u, d in zip(case["sp"]["up"], case["sp"]["dn"]) if (int(u), int(d)) == key) == m["L"] > kc["LONG_RUN"] + 64
    if "n_hii" in m:
        assert t["K_stoch"] == m["n_hii"], (case["name"], t)
    if "det_rows" in m:
        assert t["K_det"] >= m["det_rows"] and lay[m["target"] + 1]["K_det"] >= m["det_rows"], (case["name"], lay)
    return lay


# ------------------------------------------------------------------------------------------------ the child
def run_hii(blob, case):
    """matrix_elements of the targeted bucket's walkers outside the deterministic space, as the bucket tail left them"""
    res, sp, prm = case["res"], case["sp"], case["prm"]
    g = EC._ctx(blob, 1, EC.MWALK, int((res["imp_distance"] == 0).sum()))
    try:
        EC._upload(g, res)
        g.annihilate(prm, sp)
        got = g.download_walkers()
    finally:
        g.close()
    worst = 0.0
    for i, (val, bound) in case["want_me"].items():
        err = abs(float(got["matrix_elements"][i]) - val)
        worst = max(worst, err / bound)
        if not err <= bound:
            return "matrix_elements[%d] = %r, independent H %r, bound %r" % (i, float(got["matrix_elements"][i]), val, bound), worst
    return None, worst


def main(argv):
    path, variant = argv[1], argv[2]
    for k, v in EC.VARIANTS[variant][0].items():
        assert os.environ.get(k) == v, "the environment of this process does not select variant %s" % variant
    with open(path, "rb") as f:
        blob = pickle.load(f)
    import sqmc_amd
    sqmc_amd.set_device(0)
    t0 = time.time()
    n_bad = 0
    for case in blob["cases"]:
        if not case["meta"].get("rounds"):
            continue
        rec = EC.run_case(blob, variant, case)
        if rec.get("ok") and variant == "bucket" and "want_me" in case:
            why, worst = run_hii(blob, case)
            rec["hii_worst_error_over_bound"] = worst
            if why:
                rec["ok"] = False; rec["why"] = why
        print(json.dumps(rec, default=str), flush=True)
        if rec.get("status", 0) < 0:
            return 3
        n_bad += 0 if rec["ok"] else 1
    print(json.dumps(dict(variant=variant, cases_failed=n_bad, seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
