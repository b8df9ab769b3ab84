"""Directed inputs for the sort of k_anneal_bucket's short lists: the histogram over the gaps and the ranking inside a gap.

A spawn's GAP is the number of residents of its bucket with key <= its own.  The kernel counts the spawns of every gap, hands each
spawn some free place in its gap's range (whatever order the atomics make) and then ranks it among the words of its gap by
(key, slot); the cases put one bucket (meta['target']) at the places where that can go wrong.  Each case is a list of B >= 3
equal-residents buckets written with bucket_rounds_cases.Buckets; where the name speaks of creation order or of partition rows, the
spawn list is re-sequenced afterwards (any order is a valid input: the model folds what it is given).  facts() derives, from the
boundary rule alone, what the targeted bucket holds -- spawns per gap, distinct keys per gap, the words it has in every partition
row of 256 spawns -- and check_case() asserts on the CPU that the case holds what it is named for.

The child is bucket_rounds_cases.py's (it runs every case marked `rounds`, which Buckets.finish sets).
"""
import bisect

import numpy as np

import anneal_edge_cases as EC
import bucket_rounds_cases as BR


def constants():
    kc = BR.kernel_constants()
    kc["GAP_SORT_MAX_R"] = 1023          # k_anneal_bucket: gap_sort = R <= 1023, the radix sort of the words beyond
    return kc


# ------------------------------------------------------------------------------------------------ what a bucket holds
def facts(case, target, kc):
    """of the targeted bucket, from the boundary rule (B = ceil(n_all / BK_TARGET), bucket b >= 1 begins at the key of resident
    b n0 / B): R, S, spawns per gap, distinct keys per gap, creation positions and keys of its spawns, words per partition row"""
    res, sp = case["res"], case["sp"]
    n0, ns = len(res["up"]), len(sp["up"])
    B = min(-(-(n0 + ns) // kc["BK_TARGET"]), n0)
    rkeys = [(int(u), int(d)) for u, d in zip(res["up"], res["dn"])]
    assert rkeys == sorted(rkeys)
    start = [b * n0 // B for b in range(B + 1)]
    first = [rkeys[start[b]] for b in range(1, B)]
    mine = rkeys[start[target]:start[target + 1]]
    pos, keys = [], []
    for j, (u, d) in enumerate(zip(sp["up"], sp["dn"])):
        k = (int(u), int(d))
        if bisect.bisect_right(first, k) == target:
            pos.append(j); keys.append(k)
    gaps = [bisect.bisect_right(mine, k) for k in keys]
    per_gap, keys_per_gap = {}, {}
    for g, k in zip(gaps, keys):
        per_gap[g] = per_gap.get(g, 0) + 1
        keys_per_gap.setdefault(g, set()).add(k)
    rows = {}
    for j in pos:
        rows[j // kc["BK_T"]] = rows.get(j // kc["BK_T"], 0) + 1
    return dict(B=B, R=len(mine), S=len(pos), per_gap=per_gap, keys_per_gap={g: len(v) for g, v in keys_per_gap.items()}, pos=pos, keys=keys, gaps=gaps,
                rows=rows, n_rows=-(-ns // kc["BK_T"]), on_resident={g: (g > 0 and mine[g - 1] in keys_per_gap[g]) for g in keys_per_gap})


def resequence(case, order):
    """the spawn list in the order `order` (a permutation of its positions)"""
    order = np.asarray(order, np.int64)
    assert sorted(order.tolist()) == list(range(len(case["sp"]["up"])))
    case["sp"] = {k: v[order].copy() for k, v in case["sp"].items()}


def by_key(case, target, kc, gap, how):
    """re-sequence the spawns of one gap of the targeted bucket among the positions they occupy: 'descending' key order, or
    'interleaved' (smallest, largest, second smallest, ...)"""
    f = facts(case, target, kc)
    sel = [(k, j) for k, j, g in zip(f["keys"], f["pos"], f["gaps"]) if g == gap]
    srt = sorted(sel)
    if how == "descending":
        seq = srt[::-1]
    else:
        seq, lo, hi = [], 0, len(srt) - 1
        while lo <= hi:
            seq.append(srt[lo]); lo += 1
            if lo <= hi:
                seq.append(srt[hi]); hi -= 1
    order = list(range(len(case["sp"]["up"])))
    for (_, src), dst in zip(seq, sorted(j for _, j in sel)):
        order[dst] = src
    resequence(case, order)


# ------------------------------------------------------------------------------------------------ the cases
def build_cases(uu, ud, kc):
    A, TG = kc["A"], kc["BK_TARGET"]
    cases = []
    seed = [9100]
    kept_new, dropped_new = (0.75, 2, 1), (0.5, 2, 0)
    heavy = lambda n: [((0.5 if k == 0 else (0.25 if k % 2 else -0.25)), (2, 3, 1)[k % 3], (1, 0)[k % 2]) for k in range(n)]      # both signs, running weight 0.5 / 0.75

    def make(name, R, fill, target=1, **meta):
        """fill(bk) writes the targeted bucket (beginning with a resident); the others carry ordinary residents and the spawns it
        takes for exactly B buckets"""
        seed[0] += 1
        own = Buckets_probe(uu, ud, seed[0], R, fill)
        B = 3
        while B * R + (own - R) + 2 * (B - 1) > B * TG:
            B += 1
        bk = BR.Buckets(uu, ud, seed[0], B, R)
        for b in range(B):
            bk.bucket()
            if b == target:
                fill(bk)
            bk.rest()
        total = max((B - 1) * TG + 50, bk.b.slots() + 2 * (B - 1))
        assert total <= B * TG and total <= EC.MWALK
        bk.pad([b for b in range(B) if b != target], total)
        c = bk.finish(name, target=target, **meta)
        cases.append(c)
        return c

    def plain(bk, n):
        for _ in range(n):
            bk.res()

    # ---- no spawn at all, one spawn
    make("S_0", 40, lambda bk: plain(bk, 40), S=0)
    make("S_1", 40, lambda bk: (plain(bk, 17), bk.new([kept_new]), plain(bk, 23)), S=1)
    # ---- only gap 0 (the list's first bucket: keys below the first resident), only gap R (behind the bucket's last resident)
    def gap0(bk):
        for k in range(30):
            bk.b.spawn(k % 8, bk.b._w(True), 2, int(k % 3 != 0))       # the universe's first eight determinants stay free (Builder)
        plain(bk, 50)
    make("only_gap_0", 50, gap0, target=0, S=30, gaps=[0])
    make("only_gap_R", 50, lambda bk: (plain(bk, 50), [bk.new([kept_new if k % 2 else dropped_new] * (1 + k % 3)) for k in range(12)]), S=24, gaps=[50])
    # ---- several distinct free keys in one gap, created in descending / interleaved key order
    def one_gap(bk):
        plain(bk, 20)
        for k in range(9):
            bk.new([(0.25 * (1 + k % 4), 2, 1)] * (1 + k % 2))
        plain(bk, 20)
    for how in ("descending", "interleaved"):
        c = make("distinct_keys_in_one_gap_" + how, 40, one_gap, S=13, gaps=[20], distinct=9, order=how)
        by_key(c, 1, kc, 20, how)
    # ---- one determinant with many spawns: equal keys across the rounds of 64 of a wavefront, across wavefronts and across the
    #      block's rounds of BK_AT, created all over the partition rows
    for n, on_res in ((65, False), (A + 1, True), (1000, True)):
        def fill(bk, n=n, on_res=on_res):
            plain(bk, 30)
            if on_res:
                bk.res(0.5, 2, 2, spawns=heavy(n))
            else:
                bk.new(heavy(n))
            for k in range(6):
                bk.res(); bk.new([kept_new])
            plain(bk, 60 - bk.nres)
        make("one_determinant_%d_spawns" % n, 60, fill, S=n + 6, heavy=n)
    # ---- a heavy gap between many empty ones
    def heavy_gap(bk):
        plain(bk, 300)
        bk.new(heavy(200))
        for k in range(4):
            bk.new([(0.25, 2, 1)] * 10)
        plain(bk, 300)
    make("heavy_gap_among_empty_gaps", 600, heavy_gap, S=240, gaps=[300], distinct=5)
    # ---- more residents than the gap sort takes: the radix sort of the words still runs behind the same gather
    Rw = kc["GAP_SORT_MAX_R"] + 7
    assert Rw <= kc["CAP_R"]
    def wide(bk):
        for q in range(Rw):
            if q % 400 == 100:
                bk.res(spawns=[(bk.b._w(True), 2, 1)] * 2)
            elif q % 400 == 250:
                bk.res(); bk.new([kept_new])
            else:
                bk.res()
    make("wide_resident_list", Rw, wide, S=8, radix=True)
    return cases


def Buckets_probe(uu, ud, seed, R, fill):
    """slots the targeted bucket's content takes (written once into a throw-away list)"""
    bk = BR.Buckets(uu, ud, seed, 1, R)
    bk.bucket(); fill(bk); bk.rest()
    return bk.b.slots()


def check_case(case, kc):
    """CPU: the case holds what it is named for"""
    m = case["meta"]
    f = facts(case, m["target"], kc)
    assert f["B"] >= 3 and f["R"] <= kc["CAP_R"] and f["S"] <= kc["CAP_S"] and f["R"] + f["S"] <= kc["CAP_T"], (case["name"], f["B"], f["R"], f["S"])
    assert f["n_rows"] <= kc["A"], "one partition row per thread of the bucket's block"
    assert f["S"] == m["S"], (case["name"], f["S"])
    assert (f["R"] > kc["GAP_SORT_MAX_R"]) == bool(m.get("radix")), (case["name"], f["R"])
    if "gaps" in m:
        assert sorted(f["per_gap"]) == m["gaps"], (case["name"], sorted(f["per_gap"]))
        if m["gaps"] == [0]:
            assert m["target"] == 0
    if case["name"] == "only_gap_R":
        assert m["gaps"] == [f["R"]]
    if "distinct" in m:
        g = m["gaps"][0]
        assert f["keys_per_gap"][g] == m["distinct"] and not f["on_resident"][g], (case["name"], f["keys_per_gap"])
    if "order" in m:
        ks = [k for k, g in zip(f["keys"], f["gaps"]) if g == m["gaps"][0]]          # in creation order
        if m["order"] == "descending":
            assert all(a >= b for a, b in zip(ks, ks[1:])) and ks[0] > ks[-1]
        else:
            ups = sum(1 for a, b in zip(ks, ks[1:]) if a < b)
            assert ups >= 3 and len(ks) - 1 - ups >= 3, "neither ascending nor descending"
    if "heavy" in m:
        n = m["heavy"]
        g = max(f["per_gap"], key=lambda x: f["per_gap"][x])
        assert f["per_gap"][g] >= n and f["keys_per_gap"][g] <= 2
        hk = max(set(f["keys"]), key=f["keys"].count)
        where = [j for j, k in zip(f["pos"], f["keys"]) if k == hk]
        assert len(where) == n
        assert len({j // kc["BK_T"] for j in where}) >= min(f["n_rows"], 5), "created all over the partition rows"
        wts = case["sp"]["wt"][where]
        assert (wts > 0).any() and (wts < 0).any()
    if case["name"] == "heavy_gap_among_empty_gaps":
        assert f["R"] >= 500 and len(f["per_gap"]) == 1
    return f


_PREPARED = {}


def prepared(c2_walk, c2_setup, tmp_path_factory):
    """cases, model outputs and the child's file, made once per test session (the GPU test and the test of the builder share them)"""
    if not _PREPARED:
        from test_gpu_anneal_edges import tables_of, universe
        kc = constants()
        uu, ud, in_table = universe(c2_setup, n=max(3400, 5 * kc["A"] + 1500))
        ct_lib = {(int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])): (float(c2_setup.ct_num[i]), float(c2_setup.ct_den[i])) for i in in_table}
        path = str(tmp_path_factory.mktemp("gap_sort") / "cases.pkl")
        cases = [c for c in EC.prepare(path, tables_of(c2_walk), uu, ud, ct_lib, 512, build_cases(uu, ud, kc)) if c["meta"].get("rounds")]
        _PREPARED.update(kc=kc, path=path, cases=cases)
    return _PREPARED
