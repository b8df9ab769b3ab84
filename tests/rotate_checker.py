"""An independent model of the orbital rotation of the integrals,

    (PQ|RS)' = sum_abcd U_aP U_bQ U_cR U_dS (ab|cd),    h'_PQ = sum_ab U_aP U_bQ h_ab,    E_nuc' = E_nuc,

for tests of sqmc_gpu_rotate_integrals.  Nothing here comes from the HIP library, sqmc_amd/host.py or oracle/.

Orbitals are 0-based.  pair(p, q) = p (p + 1) / 2 + q for p >= q.  The canonical member of an 8-fold class (pq|rs) = (qp|rs) = (pq|sr) =
(rs|pq) = ... is the key (p, q, r, s) with p >= q, r >= s and pair(p, q) >= pair(r, s); a one-body key is (p, q) with p >= q.  Integrals
are a dict over these keys (class Integrals); a key that is absent is an exact zero.

Three ways to transform, all returning a Transformed (values and, per entry, S = sum |U_aP| |U_bQ| |U_cR| |U_dS| |(ab|cd)|):

  transform_exact    dense, in fractions.Fraction: four quarter transformations of the full tensor.  Small norb.
  transform_sparse   exact as well: every stored integral, in each of the distinct index orders of its class, is sent to the (P, Q, R, S)
                     whose four U entries are non-zero.  For U with few non-zeros per row and few integrals, at any norb.
  transform_fast     two half transformations over orbital pairs by staged np.tensordot, in np.longdouble where its mantissa has at least
                     63 bits (LONGDOUBLE_OK), in float64 otherwise; any norb up to 64 in seconds.

The bound.  A computed entry is four nested dot products of length norb.  Whatever the order of the four contractions and of the terms
inside each, with or without fused multiply-add, and also when the two inner ones are shared between entries (the half-transform
formulation: the intermediate is itself a rounded double sum, and its error passes through the outer sums multiplied by |U| |U|), the
standard bound of a nested sum applies: |computed - exact| <= gamma_{4 norb} S, gamma_k = k u / (1 - k u), u = 2^-53, which is below
4 (norb + 1) u S for norb <= 64.  So

    bound = 4 (norb + 1) 2^-53 S        (two-body),        2 (norb + 1) 2^-53 S    (one-body, two nested sums).

S itself is summed in float64 (all terms are non-negative, so the computed S is within a factor 1 +- gamma_{4 norb} of the true one) and
is multiplied by (1 + 8 (norb + 1) 2^-53) to stay an upper bound.  The longdouble reference of transform_fast carries an error of its own
of at most 4 (norb + 1) 2^-64 S, 2^-11 of the bound, which is not added; where only float64 is available the reference's error is as large
as the bound itself and the bound is counted twice (Transformed.factor = 2).  An entry with S = 0 is a sum of exact zeros and must be
exactly 0.0.

packed_index is this file's own copy of the packed 1-based addressing (pair indices from a combine_2 table that the test passes as data);
it is used only to find an entry in the array the library returned."""
import itertools
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


def pair(p, q):
    return p * (p + 1) // 2 + q if p >= q else q * (q + 1) // 2 + p


def canon(p, q, r, s):
    if p < q:
        p, q = q, p
    if r < s:
        r, s = s, r
    return (p, q, r, s) if pair(p, q) >= pair(r, s) else (r, s, p, q)


def class_members(p, q, r, s):
    """the distinct index orders of the 8-fold class of (pq|rs)"""
    return sorted({(p, q, r, s), (q, p, r, s), (p, q, s, r), (q, p, s, r), (r, s, p, q), (s, r, p, q), (r, s, q, p), (s, r, q, p)})


def canonical_keys(norb):
    """arrays P, Q, R, S of every canonical two-body key, in the order position(key) = a (a + 1) / 2 + b, a = pair(P, Q) >= b = pair(R, S)"""
    pp, qq = np.tril_indices(norb)                 # row-major lower triangle: entry k is the pair with pair(p, q) = k
    a, b = np.tril_indices(len(pp))
    return pp[a], qq[a], pp[b], qq[b]


def key_position(key):
    a, b = pair(key[0], key[1]), pair(key[2], key[3])
    return a * (a + 1) // 2 + b


class Integrals:
    """one[(p, q)] with p >= q, two[canonical key], core; absent = 0"""

    def __init__(self, norb, one=None, two=None, core=0.0):
        self.norb, self.one, self.two, self.core = norb, dict(one or {}), dict(two or {}), core
        assert all(p >= q for p, q in self.one) and all(k == canon(*k) for k in self.two)

    @classmethod
    def from_arrays(cls, norb, two_values, one_matrix, core):
        """two_values over canonical_keys(norb) in their order; one_matrix[p][q] read for p >= q"""
        P, Q, R, S = canonical_keys(norb)
        two = dict(zip(zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist()), np.asarray(two_values, float).tolist()))
        one = {(p, q): float(one_matrix[p][q]) for p in range(norb) for q in range(p + 1)}
        return cls(norb, one, two, float(core))

    def v(self, p, q, r, s):
        return self.two.get(canon(p, q, r, s), 0.0)

    def h(self, p, q):
        return self.one.get((max(p, q), min(p, q)), 0.0)

    def pair_matrix(self):
        """G[pair(p, q), pair(r, s)] = (pq|rs), symmetric, float64"""
        n = self.norb
        G = np.zeros((n * (n + 1) // 2,) * 2)
        if self.two:
            k = np.array(list(self.two.keys()), np.int64)
            a, b = k[:, 0] * (k[:, 0] + 1) // 2 + k[:, 1], k[:, 2] * (k[:, 2] + 1) // 2 + k[:, 3]
            val = np.array(list(self.two.values()), float)
            G[a, b] = val
            G[b, a] = val
        return G

    def one_matrix(self):
        H = np.zeros((self.norb, self.norb))
        for (p, q), x in self.one.items():
            H[p, q] = H[q, p] = x
        return H


class Transformed:
    """kind 'exact': two / one are dicts of Fractions over the keys with a non-zero S, two_S / one_S dicts of floats; every other entry is an
    exact zero.  kind 'fast': two, two_S arrays over canonical_keys(norb) in their order, one, one_S (norb, norb) arrays."""

    def __init__(self, kind, norb, two, two_S, one, one_S, core, factor=1):
        self.kind, self.norb, self.two, self.two_S, self.one, self.one_S, self.core, self.factor = kind, norb, two, two_S, one, one_S, core, factor

    def _inflate(self):
        return 1.0 + 8.0 * (self.norb + 1) * U53

    def value(self, p, q, r, s):
        k = canon(p, q, r, s)
        return self.two.get(k, Fraction(0)) if self.kind == "exact" else self.two[key_position(k)]

    def bound(self, p, q, r, s):
        k = canon(p, q, r, s)
        S = self.two_S.get(k, 0.0) if self.kind == "exact" else float(self.two_S[key_position(k)])
        return self.factor * 4.0 * (self.norb + 1) * U53 * S * self._inflate()

    def one_value(self, p, q):
        p, q = max(p, q), min(p, q)
        return self.one.get((p, q), Fraction(0)) if self.kind == "exact" else self.one[p, q]

    def one_bound(self, p, q):
        p, q = max(p, q), min(p, q)
        S = self.one_S.get((p, q), 0.0) if self.kind == "exact" else float(self.one_S[p, q])
        return self.factor * 2.0 * (self.norb + 1) * U53 * S * self._inflate()

    def integrals(self):
        """as Integrals (Fractions stay Fractions): the input of a second transformation"""
        if self.kind == "exact":
            return Integrals(self.norb, {k: v for k, v in self.one.items() if v != 0}, {k: v for k, v in self.two.items() if v != 0}, self.core)
        return Integrals.from_arrays(self.norb, np.asarray(self.two, float), np.asarray(self.one, float), self.core)


# ------------------------------------------------------------------------------------------------------------------------- exact, dense
def _frac_matrix(U):
    return [[Fraction(x) for x in row] for row in np.asarray(U, object).tolist()]


def transform_exact(ints, U):
    """four quarter transformations of the full tensor in Fractions (norb^5 operations each: small norb only); S on the absolute values in
    float64 by the same passes"""
    n = ints.norb
    Uf = _frac_matrix(U)
    Ua = [[abs(float(x)) for x in row] for row in Uf]
    rng = range(n)

    def passes(T, M, zero):
        for axis in range(4):
            new = {}
            for idx in itertools.product(rng, repeat=4):
                acc = zero
                for k in rng:
                    src = idx[:axis] + (k,) + idx[axis + 1:]
                    acc = acc + M[k][idx[axis]] * T[src]
                new[idx] = acc
            T = new
        return T

    T = passes({i: Fraction(ints.v(*i)) for i in itertools.product(rng, repeat=4)}, Uf, Fraction(0))
    A = passes({i: abs(float(ints.v(*i))) for i in itertools.product(rng, repeat=4)}, Ua, 0.0)
    H = {(p, q): Fraction(ints.h(p, q)) for p in rng for q in rng}
    one = {(p, q): sum((Uf[a][p] * Uf[b][q] * H[a, b] for a in rng for b in rng), Fraction(0)) for p in rng for q in range(p + 1)}
    one_S = {(p, q): sum(Ua[a][p] * Ua[b][q] * abs(float(H[a, b])) for a in rng for b in rng) for p in rng for q in range(p + 1)}
    keys = [canon(*i) for i in itertools.product(rng, repeat=4)]
    return Transformed("exact", n, {k: T[k] for k in keys}, {k: A[k] for k in keys}, one, one_S, ints.core)


# ------------------------------------------------------------------------------------------------------------------------ exact, sparse
def transform_sparse(ints, U):
    """exact for any norb when U has few non-zeros per row and the integrals are few: the work is (stored integrals) x (class members)
    x (non-zeros per row)^4.  Only keys some term reaches are stored; all others are exact zeros"""
    n = ints.norb
    Uf = _frac_matrix(U)
    rows = [[(P, Uf[a][P]) for P in range(n) if Uf[a][P] != 0] for a in range(n)]
    two, two_S, one, one_S = {}, {}, {}, {}
    for key, val in ints.two.items():
        v = Fraction(val)
        if v == 0:
            continue
        for a, b, c, d in class_members(*key):
            for (P, x), (Q, y) in itertools.product(rows[a], rows[b]):
                if P < Q:
                    continue
                for (R, z), (S_, w) in itertools.product(rows[c], rows[d]):
                    if R < S_ or pair(P, Q) < pair(R, S_):
                        continue
                    t = x * y * z * w * v
                    k = (P, Q, R, S_)
                    two[k] = two.get(k, Fraction(0)) + t
                    two_S[k] = two_S.get(k, 0.0) + abs(float(t))
    for (a0, b0), val in ints.one.items():
        v = Fraction(val)
        if v == 0:
            continue
        for a, b in sorted({(a0, b0), (b0, a0)}):
            for (P, x), (Q, y) in itertools.product(rows[a], rows[b]):
                if P < Q:
                    continue
                t = x * y * v
                one[(P, Q)] = one.get((P, Q), Fraction(0)) + t
                one_S[(P, Q)] = one_S.get((P, Q), 0.0) + abs(float(t))
    return Transformed("exact", n, two, two_S, one, one_S, ints.core)


# --------------------------------------------------------------------------------------------------------------------------------- fast
def _half(X, U, pp, qq):
    """X[p, q, m] symmetric in p, q -> Y[pair(P, Q), m] = sum_pq U[p, P] U[q, Q] X[p, q, m].  numpy has no BLAS for longdouble (64 orbitals:
    a second per 10^8 multiply-adds), but its dot releases the interpreter lock: slices of m go to eight threads, each entry is still one
    thread's sum in the same order."""
    def one(Xc):
        t = np.tensordot(U.T, Xc, axes=(1, 0))     # [P, q, m]
        t = np.tensordot(U.T, t, axes=(1, 1))      # [Q, P, m]
        return t[qq, pp, :]
    m = X.shape[2]
    if X.dtype != np.longdouble or m < 256:
        return one(X)
    cuts = [(k * m // 8, (k + 1) * m // 8) for k in range(8)]
    with ThreadPoolExecutor(8) as pool:
        return np.concatenate(list(pool.map(lambda c: one(np.ascontiguousarray(X[:, :, c[0]:c[1]])), cuts)), axis=1)


def _two_halves(G, U):
    """G[pair(p, q), pair(r, s)] -> array over canonical_keys in their order"""
    n = U.shape[0]
    pp, qq = np.tril_indices(n)
    pidx = np.zeros((n, n), np.int64)
    pidx[pp, qq] = np.arange(len(pp)); pidx[qq, pp] = np.arange(len(pp))
    Y1 = _half(G[pidx], U, pp, qq)                 # [PQ, rs]
    Y2 = _half(Y1.T[pidx], U, pp, qq)              # [RS, PQ]
    a, b = np.tril_indices(len(pp))
    return Y2[b, a]


def transform_fast(ints, U):
    n = ints.norb
    dt = np.longdouble if LONGDOUBLE_OK else np.float64
    U64 = np.asarray(U, np.float64)
    G, H = ints.pair_matrix(), ints.one_matrix()
    two = _two_halves(G.astype(dt), U64.astype(dt))
    two_S = _two_halves(np.abs(G), np.abs(U64))
    Ud = U64.astype(dt)
    one = Ud.T @ H.astype(dt) @ Ud
    one_S = np.abs(U64).T @ np.abs(H) @ np.abs(U64)
    return Transformed("fast", n, two, two_S, one, one_S, ints.core, factor=1 if LONGDOUBLE_OK else 2)


# ------------------------------------------------------------------------------------------------------------------------------ compare
def packed_index(c2, i, j, k, l):
    """1-based packed address of (ij|kl) in the library's array: pair indices a = c2[i, j], b = c2[k, l], then hi (hi - 1) / 2 + lo"""
    a, b = np.asarray(c2)[i, j].astype(np.int64), np.asarray(c2)[k, l].astype(np.int64)
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    return hi * (hi - 1) // 2 + lo


def addresses(norb, c2):
    """(two-body addresses over canonical_keys in their order, one-body addresses [norb, norb] (read for p >= q), address of the core energy)"""
    P, Q, R, S = canonical_keys(norb)
    n1 = norb + 1
    p, q = np.meshgrid(np.arange(1, n1), np.arange(1, n1), indexing="ij")
    return (packed_index(c2, P + 1, Q + 1, R + 1, S + 1), packed_index(c2, p, q, np.full_like(p, n1), np.full_like(p, n1)),
            int(packed_index(c2, np.array(n1), np.array(n1), np.array(n1), np.array(n1))))


def unaddressed(norb, c2, size):
    """boolean mask over the packed array: the slots no orbital index reaches (they must hold 0.0)"""
    two, one, core = addresses(norb, c2)
    m = np.ones(size, bool)
    m[two] = False; m[one.reshape(-1)] = False; m[core] = False
    return m


def compare(exp, got, c2):
    """the library's packed array against a Transformed: (failures, worst |delta| / bound).  A failure is (key, got, expected, bound); an entry
    with bound 0 must be exactly 0.0 and does not enter worst.  The core energy must be exp.core exactly."""
    n = exp.norb
    got = np.asarray(got, np.float64)
    a2, a1, ac = addresses(n, c2)
    fails, worst = [], 0.0
    if got[ac] != exp.core:
        fails.append(("core", float(got[ac]), exp.core, 0.0))
    P, Q, R, S = canonical_keys(n)
    g2 = got[a2]
    tri = [(p, q) for p in range(n) for q in range(p + 1)]
    if exp.kind == "exact":
        seen = np.zeros(len(g2), bool)
        items = [((k, key_position(k)), float(g2[key_position(k)]), exp.two[k], exp.bound(*k)) for k in exp.two]
        for (_, pos), _, _, _ in items:
            seen[pos] = True
        for pos in np.nonzero(~seen & (g2 != 0.0))[0]:
            fails.append(((int(P[pos]), int(Q[pos]), int(R[pos]), int(S[pos])), float(g2[pos]), 0, 0.0))
        items = [(k, x, w, b) for (k, _), x, w, b in items]
        items += [((p, q), float(got[a1[p, q]]), exp.one_value(p, q), exp.one_bound(p, q)) for p, q in tri]
        for k, x, want, b in items:
            d = abs(Fraction(x) - want)
            if b == 0.0:
                if d != 0:
                    fails.append((k, x, float(want), 0.0))
                continue
            if not d <= b:
                fails.append((k, x, float(want), b))
            worst = max(worst, float(d) / b)
        return fails, worst
    scale = exp.factor * (n + 1) * U53 * exp._inflate()
    for g, want, S_, fac, keyf in ((g2, exp.two, exp.two_S, 4.0, lambda i: (int(P[i]), int(Q[i]), int(R[i]), int(S[i]))),
                                   (np.array([got[a1[p, q]] for p, q in tri]), np.array([exp.one[p, q] for p, q in tri]),
                                    np.array([exp.one_S[p, q] for p, q in tri]), 2.0, lambda i: tri[i])):
        b = fac * scale * np.asarray(S_, np.float64)
        d = np.abs(g.astype(want.dtype) - want).astype(np.float64)
        zero = b == 0.0
        bad = np.where(zero, g != 0.0, ~(d <= b))
        for i in np.nonzero(bad)[0][:20]:
            fails.append((keyf(int(i)), float(g[i]), float(want[i]), float(b[i])))
        if (~zero).any():
            worst = max(worst, float(np.max(d[~zero] / b[~zero])))
    return fails, worst
