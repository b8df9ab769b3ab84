"""An independent model of one sample of the semistochastic Epstein-Nesbet correction (second_order_pt_alias, hci.f90:1314-1660), on
top of tests/hci_checker.py and tests/proposal_checker.py.  Nothing here comes from oracle/ or from the HIP library.

The sample.  n_mc determinants are drawn from a variational list with p_i = |c_i| / sum|c|; ids are the distinct ones (positions in
the list), counts their multiplicities w_i.  Every sampled determinant generates its connections at eps_pt; for every connected
determinant k outside the list

    term1 = sum x w/p        term2 = sum x^2 ((n_mc - 1) w/p - (w/p)^2)        x = H_ki c_i, one summand per raw excitation,

term1_big and term2_big are the same sums over the paths with |x| > eps_pt_big (strict for every excitation class:
chemistry.f90:6978, 7139, heg.f90:2703), and

    value = sum_k (term1^2 + term2 - term1_big^2 - term2_big) / (E_var - H_kk) / (n_mc (n_mc - 1)),    n_connected = number of k.

Why an exhaustive expectation is a test.  For independent draws the counts are multinomial: E[w_i w_j] = n (n-1) p_i p_j and
E[w_i^2] = n p_i + n (n-1) p_i^2, so E[term1^2 + term2] = n (n-1) (sum_i x_i)^2 for every k, and the same for the big sums.  The sum
over every multiset of draws of probability times value is therefore PT2(eps_pt) - PT2(eps_pt_big) of hci_checker.pt2, to rounding;
expectation() enumerates the multisets and fold() adds them up.

Conventions that the model fixes.
  * A path with | |x| / eps_pt_big - 1 | <= HC.BORDERLINE is borderline: it is listed and compare() refuses the case, as
    hci_checker does for the generator's own screen.  A noise path (hci_checker: an element that is zero within its rounding bound)
    that could pass the screen stands in the sums as x = 0 with its bound; a determinant that only such paths reach is optional:
    it may or may not be counted in n_connected.
  * A sampled determinant with c_i = 0 has p_i = 0 and w/p = inf; it generates nothing, so nothing reads that value.
  * time_sym=True takes the raw paths of hci_checker unmerged, with the time-reversal factors in x, as the generator's raw mode
    returns them.  Two paths of one source to one representative then stand in term2 as x'^2 + x''^2 where the identity above
    needs (x' + x'')^2, and the big mask sees x after the factors where hci_checker.pt2 screens the raw element: the estimator is
    biased there (tests/test_pt2s_checker.py measures by how much).

The bound (first order, nothing tuned).  With u = 2^-53, per path b_x = the bound hci_checker gives for x, r_w = (n_var + 8) u the
relative error of w/p (the sum of |c| in any order, two divisions, both sides), F = (n_mc - 1) w/p + (w/p)^2:
    d(x w/p) = b_x w/p + |x w/p| (r_w + 2u)          d(x^2 f) = 2 |x| b_x F + x^2 F (2 r_w + 8u)
    d term  = sum of those over the run + (L - 1) u sum|summands|            (L paths added left to right)
    d T     = 2 |term1| d term1 + 2 |term1_big| d term1_big + d term2 + d term2_big + 5u A_k,   A_k = term1^2 + |term2| + term1_big^2 + |term2_big|
    d (T / D) = d T / |D| + A_k / |D| (b_D / |D| + 2u),   D = E_var - H_kk,  b_D = H_kk's rounding bound + u (|E_var| + |H_kk|)
    bound   = sum_k d (T / D) / (n_mc (n_mc - 1)) + (K + 2) 2^-52 A,         A = sum_k A_k / |D_k| / (n_mc (n_mc - 1))
K is the longest chain of additions between a term and the sum, chain(): the device's tree over the raw connection count or numpy's
pairwise sum over the terms, whichever is longer."""
import itertools
import math
from fractions import Fraction

import numpy as np

from tests import hci_checker as HC
from tests import proposal_checker as PC

U = 2.0 ** -53
DOCTORS = ("nm1", "norm", "neighbour_w", "no_counts", "keep_var", "big_on_h", "big_true", "big_false", "split_run", "hkk_source")
_DIAG, _TABLES = {}, {}


def chain(n_raw, n_terms):
    """K: additions between a term and the sum.  Device (n_raw sorted raw connections, nb = min(ceil(n_raw / 256), 1024) blocks of
    256): ceil(n_raw / (256 nb)) grid-stride additions per thread, 6 shuffle levels, 4 wavefront partials, ceil(nb / 64) block
    partials per lane of the finishing wavefront, 6 shuffle levels.  numpy's sum over n_terms: pieces of 8192 left to right, halved
    down to leaves of 128 (6 levels at most), 15 additions in a leaf's accumulators, 3 levels to combine them, 7 trailing."""
    nb = min(-(-max(n_raw, 1) // 256), 1024)
    dev = -(-n_raw // (256 * nb)) + 6 + 4 + -(-nb // 64) + 6
    piece = min(max(n_terms, 1), 8192)
    host = (-(-n_terms // 8192) - 1) + max(0, math.ceil(math.log2(piece / 128.0))) + 15 + 3 + 7
    return max(dev, host)


def blocks(n_raw):
    return min(-(-n_raw // 256), 1024)


def diagonal(H, det, time_sym=False, z=1):
    """HC.diagonal, kept per (H, det): the entry holds H, so a collected Hamiltonian's id cannot serve another one"""
    key = (id(H), det, bool(time_sym), z)
    e = _DIAG.get(key)
    if e is None or e[0] is not H:
        e = _DIAG[key] = (H, HC.diagonal(H, det, time_sym, z))
    return e[1]


def probabilities(coeffs):
    tot = math.fsum(abs(float(c)) for c in coeffs)
    return [abs(float(c)) / tot for c in coeffs]


class Result:
    """value, n_connected, n_optional, A, bound, K, n_raw (raw connections of the sample, self slots included), longest_run, borderline,
    terms: det -> (term1, term2, term1_big, term2_big, H_kk)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def compare(res, value, n_connected):
    """(failures, |delta| / bound) of a door's sample against the model's"""
    if res.borderline:
        return [("borderline", "%d paths sit on a threshold, e.g. %s" % (len(res.borderline), res.borderline[:3]))], 0.0
    fails = []
    if not res.n_connected <= int(n_connected) <= res.n_connected + res.n_optional:
        fails.append(("count", "n_connected %d, expected %d (and up to %d that only noise paths reach)" % (n_connected, res.n_connected, res.n_optional)))
    d = abs(float(value) - res.value)
    if not d <= res.bound:
        fails.append(("value", "%r against %r, bound %.3g" % (value, res.value, res.bound)))
    return fails, (d / res.bound if res.bound > 0 else (0.0 if d == 0 else math.inf))


class Table:
    """every raw path of every live determinant of the list that passes the screen at eps_pt, self slots left out, sorted by the
    determinant it reaches (paths of one determinant in source order): the part of a sample that does not depend on the draws"""

    def __init__(self, H, var, coeffs, eps_pt, active_space, time_sym, z):
        self.H, self.ts, self.z = H, bool(time_sym), z
        self.var = [(int(a), int(b)) for a, b in var]
        self.coeffs = [float(c) for c in coeffs]
        self.p = probabilities(self.coeffs)
        inside = set(self.var)
        rows, self.borderline, self.n_raw_of = [], [], [0] * len(self.var)
        for i, (v, c) in enumerate(zip(self.var, self.coeffs)):
            if c == 0.0:
                continue
            con = HC.connections(H, [v], [c], eps_pt, 0, active_space=active_space, time_sym=time_sym, z=z)
            self.borderline += [(i, det, r) for _, det, r in con.borderline]
            self.n_raw_of[i] = len(con.raw)
            assert con.raw[0][0] == v and con.raw[0][2] == 0.0
            rows += [(det, i, x, b, False) for det, _, x, b in con.raw[1:]]
            rows += [(det, i, 0.0, b, True) for (_, det), bs in con.noise_paths.items() for b in bs]
        rows.sort(key=lambda r: r[0])                                   # stable: source order within a determinant
        self.keys = sorted({r[0] for r in rows})
        index = {k: j for j, k in enumerate(self.keys)}
        self.kid = np.array([index[r[0]] for r in rows], np.int64)
        self.src = np.array([r[1] for r in rows], np.int64)
        self.x = np.array([r[2] for r in rows], float)
        self.bx = np.array([r[3] for r in rows], float)
        self.noise = np.array([r[4] for r in rows], bool)
        self.key_inside = np.array([k in inside for k in self.keys], bool)
        self.row_inside = self.key_inside[self.kid] if len(rows) else np.zeros(0, bool)

    def _hkk(self, det):
        return diagonal(self.H, det, self.ts, self.z)

    def sample(self, ids, counts, e_var, eps_pt_big, n_mc, doctor=None):
        assert doctor is None or doctor in DOCTORS, doctor
        ids, counts = [int(i) for i in ids], [int(w) for w in counts]
        n_var, m = len(self.var), len(ids)
        if doctor == "no_counts":
            counts = [1] * m
        wop = [w / self.p[i] if self.p[i] > 0.0 else math.inf for i, w in zip(ids, counts)]
        w_var, sampled = np.zeros(n_var), np.zeros(n_var, bool)
        for k, i in enumerate(ids):
            sampled[i] = True
            w_var[i] = wop[i % m] if doctor == "neighbour_w" else wop[k]      # the position in the list taken for the one among the sampled
        sel = np.nonzero(sampled[self.src])[0] if len(self.src) else np.zeros(0, np.int64)
        if doctor != "keep_var":
            sel = sel[~self.row_inside[sel]]
        n_raw = sum(self.n_raw_of[i] for i in ids)
        empty = Result(value=0.0, n_connected=0, n_optional=0, A=0.0, bound=0.0, K=chain(n_raw, 0), n_raw=n_raw, longest_run=0, borderline=list(self.borderline), terms={})
        if len(sel) == 0:
            return empty
        x, bx, src, kid = self.x[sel], self.bx[sel], self.src[sel], self.kid[sel]
        w = w_var[src]
        nm1 = float(n_mc if doctor == "nm1" else n_mc - 1)
        a1, a2 = x * w, (x * x) * (nm1 * w - w * w)
        screened = np.abs(x / np.array(self.coeffs)[src]) if doctor == "big_on_h" else np.abs(x)
        big = screened > eps_pt_big
        if doctor == "big_true":
            big[:] = True
        if doctor == "big_false":
            big[:] = False
        borderline = list(self.borderline)
        if eps_pt_big > 0 and math.isfinite(eps_pt_big):
            for j in np.nonzero(np.abs(np.abs(x) / eps_pt_big - 1.0) <= HC.BORDERLINE)[0]:
                borderline.append((int(src[j]), self.keys[kid[j]], float(abs(x[j]) / eps_pt_big)))
        rw = (n_var + 8) * U
        F = nm1 * w + w * w
        d1 = bx * w + np.abs(a1) * (rw + 2 * U)
        d2 = 2.0 * np.abs(x) * bx * F + x * x * F * (2 * rw + 8 * U)
        head = np.ones(len(sel), bool); head[1:] = kid[1:] != kid[:-1]
        if doctor == "split_run":                                       # the second path of the longest run is taken for a head
            st = np.nonzero(head)[0]
            ln = np.diff(np.append(st, len(sel)))
            if ln.max() > 1:
                head[st[int(np.argmax(ln))] + 1] = True
        st = np.nonzero(head)[0]
        ln = np.diff(np.append(st, len(sel)))
        cols = [a1, a2, np.where(big, a1, 0.0), np.where(big, a2, 0.0)]
        sums = [np.add.reduceat(col, st) for col in cols]
        abss = [np.add.reduceat(np.abs(col), st) for col in cols]
        errs = [np.add.reduceat(col, st) for col in (d1, d2, np.where(big, d1, 0.0), np.where(big, d2, 0.0))]
        for r in np.nonzero(ln > 1)[0]:                                 # runs of more than one path: math.fsum
            a, b = int(st[r]), int(st[r] + ln[r])
            for q in range(4):
                sums[q][r] = math.fsum(cols[q][a:b].tolist())
        errs = [e + (ln - 1) * U * s for e, s in zip(errs, abss)]
        real = np.add.reduceat((~self.noise[sel]).astype(np.int64), st) > 0      # a determinant that only noise paths reach is optional
        n_optional = int((~real).sum())
        st, ln, sums, errs = st[real], ln[real], [q[real] for q in sums], [q[real] for q in errs]
        if len(st) == 0:
            empty.n_optional, empty.borderline = n_optional, borderline
            return empty
        t1, t2, t1b, t2b = sums
        dets = [self.keys[kid[a]] for a in st]
        if doctor == "hkk_source":
            diag = [self._hkk(self.var[int(src[a])]) for a in st]
        else:
            diag = [self._hkk(d) for d in dets]
        h = np.array([e[0] for e in diag])
        bh = np.array([PC.rounding_bound(e[1], e[2]) for e in diag]) + U * (abs(e_var) + np.abs(h))
        den = e_var - h
        Ak = t1 * t1 + np.abs(t2) + t1b * t1b + np.abs(t2b)
        T = t1 * t1 + t2 - t1b * t1b - t2b
        dT = 2.0 * np.abs(t1) * errs[0] + 2.0 * np.abs(t1b) * errs[2] + errs[1] + errs[3] + 5 * U * Ak
        dterm = dT / np.abs(den) + Ak / np.abs(den) * (bh / np.abs(den) + 2 * U)
        norm = float(n_mc) * (n_mc if doctor == "norm" else n_mc - 1)
        value = math.fsum((T / den).tolist()) / norm
        A = math.fsum((Ak / np.abs(den)).tolist()) / norm
        K = chain(n_raw, len(st))
        bound = math.fsum(dterm.tolist()) / norm + (K + 2) * 2 * U * A
        terms = {d: (float(t1[r]), float(t2[r]), float(t1b[r]), float(t2b[r]), float(h[r])) for r, d in enumerate(dets)}
        return Result(value=value, n_connected=len(st), n_optional=n_optional, A=A, bound=bound, K=K, n_raw=n_raw, longest_run=int(ln.max()),
                      borderline=borderline, terms=terms)


def table(H, var, coeffs, eps_pt, active_space=None, time_sym=False, z=1):
    key = (id(H), tuple((int(a), int(b)) for a, b in var), tuple(float(c) for c in coeffs), float(eps_pt), active_space, bool(time_sym), z)
    t = _TABLES.get(key)
    if t is None or t.H is not H:
        t = _TABLES[key] = Table(H, var, coeffs, eps_pt, active_space, time_sym, z)
    return t


def sample(H, var, coeffs, ids, counts, e_var, eps_pt, eps_pt_big, n_mc, active_space=None, time_sym=False, z=1, doctor=None):
    """one sample by brute force: a Result.  ids: 0-based positions in var, counts: their multiplicities.  doctor: one of DOCTORS,
    a mistake built into a copy of the model (for the self-test of the comparison's power)"""
    return table(H, var, coeffs, eps_pt, active_space, time_sym, z).sample(ids, counts, e_var, eps_pt_big, n_mc, doctor)


# ---------------------------------------------------------------------------------------------- the exhaustive expectation
def expectation(coeffs, n_mc):
    """every multiset of n_mc draws over the determinants with p_i > 0: yields (ids ascending, counts, probability), the
    multinomial probability n! / prod w_i! prod p_i^w_i from the model's own p, exact in rationals and rounded once"""
    p = probabilities(coeffs)
    live = [i for i, q in enumerate(p) if q > 0.0]
    for combo in itertools.combinations_with_replacement(live, n_mc):
        ids = sorted(set(combo))
        counts = [combo.count(i) for i in ids]
        P = Fraction(math.factorial(n_mc))
        for i, w in zip(ids, counts):
            P = P * Fraction(p[i]) ** w / math.factorial(w)
        yield ids, counts, float(P)


def fold(probs, values, bounds, As, n_var, n_mc):
    """(sum P v, its bound): sum P bound, and on top what the probabilities themselves carry -- each is rounded once and the p_i
    add up to 1 only within n_var u, so the weights of n_mc draws are off by n_mc (n_var + 2) u relatively -- applied to sum P A"""
    v = math.fsum(P * x for P, x in zip(probs, values))
    b = math.fsum(P * x for P, x in zip(probs, bounds)) + (n_mc * (n_var + 2) + 2) * U * math.fsum(P * a for P, a in zip(probs, As))
    return v, b


# ---------------------------------------------------------------------------------------------- from a raw list handed in
def from_raw(cu, cd, x, src, var, wop, e_var, h_kk_of, eps_pt_big, n_mc, n_var=None, h_bound=0.0):
    """The same sums from a raw connection list as the generator's raw mode returns it (generation order, src = index of the
    source among the sampled determinants, self slots included), for shapes the brute force cannot reach.  The list is sorted by
    determinant (stable), determinants of var are dropped, and within a run the summands are added left to right in the list's
    order -- the operations and the order the device uses, so a run's four sums carry its bits; math.fsum across runs.
    h_kk_of(up array, dn array) -> H_kk array; h_bound: what those values may differ by from the device's own.
    The bound is (K + 2) 2^-52 A plus the first-order effect of w/p (relative (n_var + 8) u, propagated as in sample()) and of h_bound.
    Result has, besides the fields of sample(): run_lengths (every run of the sorted list, members of var included),
    crosses_256 / crosses_stride: sorted positions of the heads of runs that reach across a multiple of 256 / 262144,
    starts_on_stride: heads that sit on a multiple of 262144 (other than 0); n_paths, n_big: connections to determinants outside
    var, and those of them above eps_pt_big."""
    cu, cd = np.asarray(cu, np.uint64), np.asarray(cd, np.uint64)
    x, src, wop = np.asarray(x, float), np.asarray(src).astype(np.int64), np.asarray(wop, float)
    n_raw = len(cu)
    o = np.lexsort((cd, cu))
    cu, cd, x, src = cu[o], cd[o], x[o], src[o]
    head = np.ones(n_raw, bool); head[1:] = (cu[1:] != cu[:-1]) | (cd[1:] != cd[:-1])
    st = np.nonzero(head)[0]
    ln = np.diff(np.append(st, n_raw))
    last = st + ln - 1
    info = dict(run_lengths=ln, crosses_256=st[(st // 256) != (last // 256)], crosses_stride=st[(st // 262144) != (last // 262144)],
                starts_on_stride=st[(st % 262144 == 0) & (st > 0)])
    inside = set((int(a), int(b)) for a, b in var)
    keep = np.array([(int(cu[a]), int(cd[a])) not in inside for a in st], bool)
    st0, st, ln = st, st[keep], ln[keep]
    n_var = len(var) if n_var is None else n_var
    if len(st) == 0:
        return Result(value=0.0, n_connected=0, n_optional=0, A=0.0, bound=0.0, K=chain(n_raw, 0), n_raw=n_raw, longest_run=0, borderline=[], terms={}, **info)
    w = wop[src]
    nm1 = float(n_mc - 1)
    a1, a2 = x * w, (x * x) * (nm1 * w - w * w)
    big = np.abs(x) > eps_pt_big
    borderline = []
    if eps_pt_big > 0 and math.isfinite(eps_pt_big):
        borderline = [(int(src[j]), (int(cu[j]), int(cd[j])), float(abs(x[j]) / eps_pt_big))
                      for j in np.nonzero(np.abs(np.abs(x) / eps_pt_big - 1.0) <= HC.BORDERLINE)[0]]
    a1b, a2b = np.where(big, a1, 0.0), np.where(big, a2, 0.0)
    member = np.repeat(keep, np.diff(np.append(st0, n_raw)))             # per connection: its determinant is outside var
    info.update(n_paths=int(member.sum()), n_big=int((big & member).sum()))
    t = [col[st].copy() for col in (a1, a2, a1b, a2b)]
    for r in np.nonzero(ln > 1)[0]:
        for q, col in enumerate((a1, a2, a1b, a2b)):
            acc = float(col[st[r]])
            for j in range(int(st[r]) + 1, int(st[r] + ln[r])):
                acc = acc + float(col[j])
            t[q][r] = acc
    t1, t2, t1b, t2b = t
    h = np.asarray(h_kk_of(cu[st], cd[st]), float)
    den = e_var - h
    Ak = t1 * t1 + np.abs(t2) + t1b * t1b + np.abs(t2b)
    T = t1 * t1 + t2 - t1b * t1b - t2b
    norm = float(n_mc) * (n_mc - 1)
    value = math.fsum((T / den).tolist()) / norm
    A = math.fsum((Ak / np.abs(den)).tolist()) / norm
    K = chain(n_raw, len(st))
    rw = (n_var + 8) * U
    F = nm1 * w + w * w
    d1, d2 = np.abs(a1) * rw, x * x * F * (2 * rw)
    D1, D2, D1b, D2b = (np.add.reduceat(col, st0)[keep] for col in (d1, d2, np.where(big, d1, 0.0), np.where(big, d2, 0.0)))
    dT = 2.0 * np.abs(t1) * D1 + 2.0 * np.abs(t1b) * D1b + D2 + D2b
    bound = (K + 2) * 2 * U * A + math.fsum(((dT + Ak * (h_bound / np.abs(den))) / np.abs(den)).tolist()) / norm
    return Result(value=value, n_connected=len(st), n_optional=0, A=A, bound=bound, K=K, n_raw=n_raw, longest_run=int(ln.max()), borderline=borderline,
                  terms={}, **info)
