"""An independent model of the bucket-boundary blocks (sqmc_amd/csrc/bucket_partition.h), restated from their comments, and the
cases tests/test_gpu_bucket_boundaries.py puts through the door sqmc_gpu_debug_bucket_boundaries.

Nothing here searches the way the kernel does: positions come from np.searchsorted, the prefix of the bucket costs from a Python loop
in float64 (left to right, as the kernel's one thread adds them), the bucket a target falls into and the partition point inside it
from LINEAR scans.  Integers throughout, so agreement with the device is exact.
"""
import numpy as np

SPAWN_COST = 1.2          # BK_REBAL_SPAWN_COST: a spawn against a resident in a bucket's cost
RESIDENTS_MAX = 1000      # BK_RESIDENTS_MAX: boundaries that would put more residents into a bucket are not used
M32 = 0xFFFFFFFF


def _u32_of_double(x):
    """the device's conversion of a double to an unsigned 32-bit word: truncation, saturating at both ends"""
    if not x > 0.0:
        return 0
    return M32 if x >= 4294967296.0 else int(x)


def positions(keys, B, kb):
    """pos[j] = first position of the ascending list `keys` whose key is >= kb[j]; pos[0] = 0 and pos[B] = len(keys) whatever kb holds.
    (The hint only tells the kernel where to look first: it cannot change the answer.)"""
    keys = np.asarray(keys, np.uint32)
    pos = np.searchsorted(keys, np.asarray(kb, np.uint32), "left").astype(np.uint32)
    pos[0], pos[B] = 0, len(keys)
    return pos


def admitted(m, keys, p_lo, K_lo, d, r):
    """does the cost up to resident m (exclusive) of an old bucket still fit under r?  cost = (m - p_lo) + d (key(m) - K_lo)"""
    km = int(keys[m])
    return float(m - p_lo) + d * float(km - K_lo if km > K_lo else 0) <= r


def partition_point_linear(keys, p_lo, p_hi, K_lo, d, r):
    a = p_lo
    while a < p_hi and admitted(a, keys, p_lo, K_lo, d, r):
        a += 1
    return a


def partition_point_bisect(keys, p_lo, p_hi, K_lo, d, r):
    a, e = p_lo, p_hi
    while a < e:
        m = (a + e) >> 1
        if admitted(m, keys, p_lo, K_lo, d, r):
            a = m + 1
        else:
            e = m
    return a


def next_boundaries(keys, B, kb_prev, pos_prev, scount, point=partition_point_linear):
    """(kb_out[B], hint_out[B], info): the next boundaries -- every bucket the same cost (residents + SPAWN_COST spawns), if residents
    and spawns fall as they did when scount was taken, the spawns evenly over the key range of each bucket of then.  info: which
    rules fired (the tests assert that a case meets the rule it was built for)."""
    keys = np.asarray(keys, np.uint32)
    n0 = len(keys)
    prev = kb_prev is not None and pos_prev is not None
    pp, kk = [0] * (B + 1), [0] * (B + 1)
    for j in range(B + 1):
        # the boundaries of then, where they lay then (without them: equal numbers of residents); a list that shrank clamps them
        p = 0 if j == 0 else n0 if j == B else int(pos_prev[j]) if prev else (j * n0) // B
        p = min(p, n0)
        pp[j] = p
        kk[j] = 0 if j == 0 else (int(keys[n0 - 1]) + 1) & M32 if j == B else int(kb_prev[j]) if prev else int(keys[min(p, n0 - 1)])
    pre, acc = [], 0.0
    for b in range(B):
        pre.append(acc)
        acc = acc + (float((pp[b + 1] - pp[b]) & M32) + SPAWN_COST * float(int(scount[b])))
    pre.append(acc)
    total = acc
    kn, pn = [0] * (B + 1), [0] * (B + 1)
    kn[B], pn[B] = kk[B], n0
    info = dict(front=0, behind=0, d_zero=0, k_equal=0, empty_old=0, clamped=int(prev and any(int(pos_prev[j]) > n0 for j in range(1, B))),
                searched=set(), bad=False, too_many=False, first_empty=False, last_empty=False, disorder=False)
    for j in range(1, B):
        target = total * float(j) / float(B)
        lo = 0
        for b in range(B):                      # the old bucket the target falls into: the last whose prefix is <= target
            if pre[b] <= target:
                lo = b
        r = target - pre[lo]
        p_lo, p_hi, K_lo, K_hi = pp[lo], pp[lo + 1], kk[lo], kk[lo + 1]
        d = SPAWN_COST * float(int(scount[lo])) / float(K_hi - K_lo) if K_hi > K_lo else 0.0
        a = point(keys, p_lo, p_hi, K_lo, d, r)
        info["searched"].add(max(p_hi - p_lo, 0))
        info["k_equal"] += K_hi == K_lo
        info["d_zero"] += K_hi > K_lo and int(scount[lo]) == 0
        info["empty_old"] += p_lo >= p_hi
        info["front"] += a == p_lo and p_lo < p_hi
        info["behind"] += a == p_hi and p_lo < p_hi
        if a == p_lo:                           # in front of the bucket's first resident: as far into the gap as the spawn density allows
            k = (K_lo + (_u32_of_double(r / d) if d > 0.0 else 0)) & M32
        else:                                   # behind the last resident the cost admits, then on into the gap behind it
            kp = int(keys[a - 1])
            f = float(a - 1 - p_lo) + d * float(kp - K_lo if kp > K_lo else 0)
            k = (kp + 1 + (_u32_of_double((r - f) / d) if d > 0.0 else 0)) & M32
        cap = int(keys[a]) if a < p_hi else K_hi      # not past the first resident that was not admitted
        kn[j], pn[j] = min(k, cap), a
    # not used: boundaries out of order, more than RESIDENTS_MAX residents in a bucket, a first or last bucket without any
    for j in range(B):
        res = (pn[j + 1] - pn[j]) & M32
        if j > 0 and (kn[j] <= kn[j - 1] or pn[j] < pn[j - 1]):
            info["disorder"] = True
        if res > RESIDENTS_MAX:
            info["too_many"] = True
        if j == 0 and res == 0:
            info["first_empty"] = True
        if j == B - 1 and res == 0:
            info["last_empty"] = True
    info["bad"] = bad = info["disorder"] or info["too_many"] or info["first_empty"] or info["last_empty"]
    if bad:                                     # equal numbers of residents instead
        kb_out = [0] + [int(keys[(j * n0) // B]) for j in range(1, B)]
        hint_out = [(j * n0) // B for j in range(B)]
    else:
        kb_out, hint_out = [0] + kn[1:B], pn[:B]
    return np.array(kb_out, np.uint32), np.array(hint_out, np.uint32), info


# ------------------------------------------------------------------------------------------------ cases
def base_case(n0, B, seed, spread=2000, dup=False):
    """a resident list of n0 ascending keys, last step's boundaries at equal numbers of residents with where they lay, random
    spawn counts, and today's boundaries = last step's with exact hints"""
    rng = np.random.default_rng(seed)
    if dup:
        keys = np.sort(rng.integers(1000, 1000 + max(n0 // 3, 2), n0)).astype(np.uint32)      # runs of equal keys
    else:
        keys = np.sort(rng.choice(np.arange(1000, 1000 + 64 * n0, dtype=np.int64), n0, replace=False)).astype(np.uint32)
    kb = np.zeros(B + 1, np.uint32)
    for j in range(1, B):
        kb[j] = keys[(j * n0) // B]
    kb[B] = M32
    pos = positions(keys, B, kb)
    scount = rng.integers(0, spread, B + 1).astype(np.uint32)
    scount[B] = n0
    return dict(keys=keys, B=B, kb=kb.copy(), hint=pos.copy(), kb_prev=kb.copy(), pos_prev=pos.copy(), scount=scount)


def _with(c, **kw):
    c = dict(c)
    c.update(kw)
    return c


def cases():
    """name -> (case, rules of next_boundaries' info that must have fired)"""
    out = {}
    for B in (2, 3, 17, 256):
        out["B%d_n256" % B] = (base_case(256, B, 10 + B), ())
        out["B%d_odd" % B] = (base_case({2: 1999, 3: 2999, 17: 3001, 256: 5003}[B], B, 20 + B), ())
    c = base_case(3001, 17, 3)
    for off in (0, 383, -383, 384, -384, 385, -385):
        out["hint%+d" % off] = (_with(c, hint=np.clip(c["hint"].astype(np.int64) + off, 0, M32).astype(np.uint32)), ())
    out["hint_far_low"] = (_with(c, hint=np.zeros(18, np.uint32)), ())
    out["hint_far_high"] = (_with(c, hint=np.full(18, 3000, np.uint32)), ())
    out["hint_past_end"] = (_with(c, hint=np.full(18, 3001 + 5000, np.uint32)), ())
    out["no_hint"] = (_with(c, hint=None), ())
    kb = c["kb"].copy(); kb[1] = 0; kb[2] = 999; kb[16] = M32; kb[15] = c["keys"][-1] + 1
    out["kb_outside"] = (_with(c, kb=kb), ())
    kb = c["kb"].copy(); kb[3] = c["keys"][0]; kb[4] = c["keys"][-1]; kb[5] = c["keys"][700] + 1
    out["kb_on_and_between"] = (_with(c, kb=kb), ())
    out["dup_keys"] = (base_case(3001, 17, 4, dup=True), ())
    out["no_kb"] = (_with(c, kb=None, hint=None), ())
    out["no_prev"] = (_with(c, kb_prev=None, pos_prev=None), ())
    out["no_kb_prev"] = (_with(c, kb_prev=None), ())
    out["no_pos_prev"] = (_with(c, pos_prev=None), ())
    sc = c["scount"].copy(); sc[4] = 0; sc[5] = 0
    out["zero_spawns"] = (_with(c, scount=sc), ("d_zero",))
    kp, pv = c["kb_prev"].copy(), c["pos_prev"].copy(); kp[6] = kp[5]; pv[6] = pv[5]; sc = c["scount"].copy(); sc[5] = 4000
    out["k_equal_and_empty_old"] = (_with(c, kb_prev=kp, pos_prev=pv, scount=sc), ("k_equal", "empty_old"))
    # an old bucket whose key range begins far in front of its first resident, full of spawns: targets fall into the gap
    kp = c["kb_prev"].copy(); kp[8] = c["keys"][c["pos_prev"][7] + 1] + 1; sc = c["scount"].copy(); sc[8] = 60000
    keys = c["keys"].copy(); keys[c["pos_prev"][8]:] += 500000
    out["front_of_first"] = (_with(c, keys=keys, kb=None, hint=None, kb_prev=kp, scount=sc), ("front",))
    # ... and one whose spawns lie behind its last resident
    kp = c["kb_prev"].copy(); keys = c["keys"].copy(); keys[c["pos_prev"][9]:] += 500000; kp[9:17] += 500000; kp[9] -= 400000
    sc = c["scount"].copy(); sc[8] = 60000
    out["behind_last"] = (_with(c, keys=keys, kb=None, hint=None, kb_prev=kp, scount=sc), ("behind",))
    pv = c["pos_prev"].copy(); pv[15] = 3001 + 7; pv[16] = 3001 + 90
    out["list_shrank"] = (_with(c, pos_prev=pv), ("clamped",))
    out["too_many_residents"] = (base_case(5000, 3, 5), ("too_many",))
    # first bucket empty: the keys begin far above 0 and the first old bucket is full of spawns; last bucket empty: nearly all the
    # cost sits in a last old bucket that holds one resident
    c2 = base_case(1500, 5, 6)
    sc = c2["scount"].copy(); sc[:5] = (200000, 10, 10, 10, 10)
    out["first_empty"] = (_with(c2, keys=c2["keys"] + np.uint32(1 << 30), kb_prev=np.where(np.arange(6) % 5 == 0, c2["kb_prev"], c2["kb_prev"] + np.uint32(1 << 30)), scount=sc),
                          ("first_empty",))
    kp, pv = c2["kb_prev"].copy(), c2["pos_prev"].copy(); kp[4] = c2["keys"][-1] - 1; pv[4] = positions(c2["keys"], 5, kp)[4]
    sc = c2["scount"].copy(); sc[:5] = (0, 0, 0, 0, 100000)
    out["last_empty"] = (_with(c2, kb_prev=kp, pos_prev=pv, scount=sc), ("last_empty",))
    # old buckets of 15, 16, 17, 255, 256 and 257 residents (where a search over them gains or loses a level), every one of them searched
    sizes = [15, 16, 17, 255, 256, 257, 300, 300]
    n0 = sum(sizes)
    for s in range(3):
        c3 = base_case(n0, 8, 30 + s)
        pv = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        kp = np.zeros(9, np.uint32); kp[1:8] = c3["keys"][pv[1:8]]; kp[8] = M32
        cost = 700.0 + 40 * s
        sc = np.array([int((cost * (1.5 if b == 0 else 1.0) - sizes[b]) / SPAWN_COST) for b in range(8)] + [n0], np.uint32)      # target j falls into old bucket j - 1
        out["seams_%d" % s] = (_with(c3, kb=kp.copy(), hint=pv.copy(), kb_prev=kp, pos_prev=pv, scount=sc), ("seams",))
    return out
