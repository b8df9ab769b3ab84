"""An independent model for the O(N) diagonal update (get_new_diag_elem, chemistry.f90:9649-9739; get_new_diag_elem_heg,
heg.f90:3357-3453), on top of tests/proposal_checker.py and tests/hci_checker.py.  Nothing here comes from oracle/ or from the
HIP library.

Two things are modelled.

  * brute(H, det): H_aa from scratch by second quantisation (hci_checker.diagonal): every operator string of H applied to the
    determinant, summed with math.fsum.  This is what an update is judged against.

  * update(ints, norb, old_diag, (p, q, r, s), new_up, new_dn): the reference's statements, one floating-point operation after
    the other, left to right, in plain Python floats -- the value the library's one-lane form has to reproduce bit for bit.
    p, q, r, s are the reference's spin orbitals: 1..norb up, norb+1..2 norb dn; r has p's spin and s has q's.  It also
    returns the sum of |every integral it added or subtracted| and the number of additions it made.

The rounding bound of an update against the brute force:

    bound = gamma_k (|old_diag| + sum |every integral added or subtracted|),   gamma_k = k u / (1 - k u),  u = 2^-53,
    k = 4 + 2 + 2 + 8 n_elec

k is counted from the formula, not fitted: 4 additions in the one-body statement, 2 in the direct, 2 in the exchange statement,
and in the loops at most 4 (direct) + 4 (exchange) per occupied orbital.  The loops skip r and s and take only the exchange
branches of the right spin, so an update makes at most 8 n_elec - 8 additions; the 16 that k keeps on top cover the roundings
that are not additions of the formula: old_diag itself (one rounding of the source's element), the brute-force value (one
rounding of the exact sum) and, for the electron gas, the few-ulp difference between the integrals as the library forms them
(4 pi / (|k_i - k_j|^2 L^3) from floating k vectors) and as the checker does (1 / (pi L |n_i - n_j|^2) from integers).

Doctored updates (doctor=...) must fall outside that bound: 'exchange_branch' takes the O(1) exchange term for opposite spins
and drops it for equal ones, 'keep_r' does not skip r in the loops, 'swap_pr' exchanges the roles of p and r."""
import math

import numpy as np

from tests import hci_checker as HC
from tests import proposal_checker as PC

U = 2.0 ** -53


def n_additions(nelec):
    return 4 + 2 + 2 + 8 * nelec


def gamma(k):
    return k * U / (1.0 - k * U)


def bound(old_diag, sum_abs, nelec):
    return gamma(n_additions(nelec)) * (abs(old_diag) + sum_abs)


# ---------------------------------------------------------------------------------------------- integral_value, spatial 1-based
class ChemInts:
    """integral_value of chemistry.f90 from the checker's FCIDUMP tables: one(i) = h_ii, direct(i,j) = (ii|jj), exchange = (ij|ji);
    tabulated once (a record of the C2 system looks up about 70 of them)"""

    def __init__(self, H):
        n = H.norb
        self._one = [0.0] + [H.t(i, i) for i in range(n)]
        self._dir = [[0.0] * (n + 1)] + [[0.0] + [H.v(i, i, j, j) for j in range(n)] for i in range(n)]
        self._exc = [[0.0] * (n + 1)] + [[0.0] + [H.v(i, j, j, i) for j in range(n)] for i in range(n)]

    def one(self, i):
        return self._one[i]

    def direct(self, i, j):
        return self._dir[i][j]

    def exchange(self, i, j):
        return self._exc[i][j]


class HegInts:
    """the integrals of hamiltonian_heg from the floating k vectors and the cell length a context is given, operation by operation
    as heg.f90 forms them: one = sum(k^2) / 2 (:3471), direct = 0 (the background), exchange = 4 pi / (sum((k_j - k_i)^2) L^3) (:3482-3483)"""

    def __init__(self, k_vectors, length_cell):
        self.k = [[float(x) for x in row[:3]] for row in np.asarray(k_vectors, float)]
        self.L = float(length_cell)

    def one(self, i):
        s = 0.0
        for x in self.k[i - 1]:
            s = s + x * x
        return s * 0.5

    def direct(self, i, j):
        return 0.0

    def exchange(self, i, j):
        if i == j:
            return 0.0                  # "if (p == q) then integral_value = 0", heg.f90:3465; no valid record gets here
        s = 0.0
        for a, b in zip(self.k[i - 1], self.k[j - 1]):
            d = b - a
            s = s + d * d
        L = self.L
        return (4.0 * (4.0 * math.atan(1.0))) / (s * (L * L * L))


def ints_of(H, hsys=None):
    return HegInts(hsys.k_vectors(), hsys.length_cell) if isinstance(H, PC.HegH) else ChemInts(H)


# ---------------------------------------------------------------------------------------------- the update, statement by statement
class _Acc:
    def __init__(self, v):
        self.v, self.s, self.k = v, 0.0, 0

    def add(self, x):
        self.v = self.v + x; self.s += abs(x); self.k += 1

    def sub(self, x):
        self.v = self.v - x; self.s += abs(x); self.k += 1


def update(ints, norb, old_diag, pqrs, new_up, new_dn, doctor=None):
    """(new_diag_elem, sum |integrals used|, additions made)"""
    p_in, q_in, r_in, s_in = (int(x) for x in pqrs)
    if doctor == "swap_pr":
        p_in, r_in = r_in, p_in
    p_up, q_up = p_in <= norb, q_in <= norb
    p = p_in if p_up else p_in - norb
    q = q_in if q_up else q_in - norb
    r = r_in - norb if r_in > norb else r_in
    s = s_in - norb if s_in > norb else s_in
    occ_up = [b + 1 for b in PC._bits(int(new_up))]
    occ_dn = [b + 1 for b in PC._bits(int(new_dn))]
    a = _Acc(float(old_diag))
    a.add(ints.one(r)); a.add(ints.one(s)); a.sub(ints.one(p)); a.sub(ints.one(q))                      # :9697
    a.add(ints.direct(r, s)); a.sub(ints.direct(p, q))                                                  # :9700
    same = p_up == q_up
    if (not same) if doctor == "exchange_branch" else same:                                             # :9703
        a.sub(ints.exchange(r, s)); a.add(ints.exchange(p, q))
    skip_r = doctor != "keep_r"
    for i in occ_up:                                                                                    # :9710-9714
        if (skip_r and i == r_in) or i == s_in:
            continue
        a.add(ints.direct(i, r)); a.add(ints.direct(i, s)); a.sub(ints.direct(i, p)); a.sub(ints.direct(i, q))
    for i in occ_dn:                                                                                    # :9715-9719
        if (skip_r and i == r_in - norb) or i == s_in - norb:
            continue
        a.add(ints.direct(i, r)); a.add(ints.direct(i, s)); a.sub(ints.direct(i, p)); a.sub(ints.direct(i, q))
    if p_up or q_up:                                                                                    # :9722-9729
        for i in occ_up:
            if (skip_r and i == r_in) or i == s_in:
                continue
            if p_up:
                a.sub(ints.exchange(i, r)); a.add(ints.exchange(i, p))
            if q_up:
                a.sub(ints.exchange(i, s)); a.add(ints.exchange(i, q))
    if (not p_up) or (not q_up):                                                                        # :9730-9737
        for i in occ_dn:
            if (skip_r and i == r_in - norb) or i == s_in - norb:
                continue
            if not p_up:
                a.sub(ints.exchange(i, r)); a.add(ints.exchange(i, p))
            if not q_up:
                a.sub(ints.exchange(i, s)); a.add(ints.exchange(i, q))
    return a.v, a.s, a.k


# ---------------------------------------------------------------------------------------------- brute force and records
_CACHES = {}


def _cache(H):
    """the tables and diagonal elements already worked out for this very Hamiltonian.  The entry holds H itself: while it is
    there H cannot be collected, so its id cannot pass to another object, and the identity test says so outright (an entry keyed
    by a bare id() once served a new Hamiltonian the tables of a collected one)."""
    e = _CACHES.get(id(H))
    if e is None or e[0] is not H:
        e = _CACHES[id(H)] = (H, {}, {})
    return e


def brute(H, det):
    """H_aa from scratch by second quantisation: (value, number of terms, sum |terms|); cached per (H, det)"""
    diag = _cache(H)[1]
    key = (int(det[0]), int(det[1]))
    if key not in diag:
        diag[key] = HC.diagonal(H, key)
    return diag[key]


def brute_many(H, dets):
    """brute() for many determinants at once.  On |I> itself the operator strings of H that end in |I> again are a+_P a_P for
    every occupied P and, from 1/2 a+_P a+_R a_S a_Q, the two pairings (P, R) = (Q, S) and (P, R) = (S, Q) of every ordered
    occupied pair Q != S, with signs + and -:
        H_aa = const + sum_P t(P,P) + 1/2 sum_{Q != S} [v(Q,Q,S,S) - v(S,Q,Q,S)]
    over spin orbitals, t and v being the checker's own (proposal_checker).  Evaluated in 80-bit extended precision and rounded
    once, so the result is the correctly rounded sum up to a part in 2^11 of an ulp, as brute()'s math.fsum is; the CPU tests
    compare the two.  (brute() costs about 1 ms per determinant, the C2 records of the GPU test are 84 000.)"""
    assert np.finfo(np.longdouble).eps < 2e-19, "needs the 80-bit long double"
    tables = _cache(H)[2]
    if "TG" not in tables:
        m = 2 * H.norb
        T = np.array([H.t(P, P) for P in range(m)], np.longdouble)
        G = np.array([[0.0 if Q == S else H.v(Q, Q, S, S) - H.v(S, Q, Q, S) for S in range(m)] for Q in range(m)], np.longdouble)
        tables["TG"] = (T, G)
    T, G = tables["TG"]
    m = 2 * H.norb
    out = np.empty(len(dets))
    for a in range(0, len(dets), 4096):
        st = np.array([H.state(u, d) for u, d in dets[a:a + 4096]], dtype=object)
        N = np.array([[(int(x) >> P) & 1 for P in range(m)] for x in st], np.longdouble)
        out[a:a + 4096] = (np.longdouble(H.const) + N @ T + np.longdouble(0.5) * ((N @ G) * N).sum(axis=1)).astype(np.float64)
    return out


def apply(source, pqrs, norb):
    """the determinant p, q -> r, s leads to from source, or None when p or q is empty or r or s occupied there"""
    up, dn = int(source[0]), int(source[1])
    for k, o in enumerate(pqrs):
        is_up = o <= norb
        b = 1 << ((o if is_up else o - norb) - 1)
        cur = up if is_up else dn
        if k < 2:
            if not cur & b:
                return None
            cur ^= b
        else:
            if cur & b:
                return None
            cur |= b
        up, dn = (cur, dn) if is_up else (up, cur)
    return up, dn


def record_of(source, new, norb):
    """(p, q, r, s) of the double excitation source -> new: same spin p < q and r < s; opposite spins p, r up and q, s dn"""
    gone_u, gone_d = PC._bits(source[0] & ~new[0]), PC._bits(source[1] & ~new[1])
    came_u, came_d = PC._bits(new[0] & ~source[0]), PC._bits(new[1] & ~source[1])
    assert len(gone_u) + len(gone_d) == 2 and len(came_u) == len(gone_u) and len(came_d) == len(gone_d)
    if len(gone_u) == 2:
        return gone_u[0] + 1, gone_u[1] + 1, came_u[0] + 1, came_u[1] + 1
    if len(gone_d) == 2:
        return gone_d[0] + 1 + norb, gone_d[1] + 1 + norb, came_d[0] + 1 + norb, came_d[1] + 1 + norb
    return gone_u[0] + 1, gone_d[0] + 1 + norb, came_u[0] + 1, came_d[0] + 1 + norb


def double_records(H, source):
    """every double excitation of source as [(pqrs, new)]: chemistry all of them (the update does not ask whether H connects
    the pair), electron gas the momentum-conserving ones (proposal_checker.excitations_heg)"""
    up, dn = int(source[0]), int(source[1])
    norb = H.norb
    if isinstance(H, PC.HegH):
        news = [(nu, nd) for nu, nd in PC.excitations_heg(H, up, dn)]
    else:
        news = [(nu, nd) for nu, nd in PC.excitations_chem(up, dn, norb) if PC._pop(up & ~nu) + PC._pop(dn & ~nd) == 2]
    return [(record_of((up, dn), n, norb), n) for n in news]


def seeded_sources(hf, norb, nup, ndn, n, seed=20160309):
    """hf and n - 1 determinants with orbitals drawn without replacement from a fixed seed"""
    rng = np.random.default_rng(seed)
    out = [(int(hf[0]), int(hf[1]))]
    while len(out) < n:
        u = sum(1 << int(o) for o in rng.choice(norb, nup, replace=False))
        d = sum(1 << int(o) for o in rng.choice(norb, ndn, replace=False))
        if (u, d) not in out:
            out.append((u, d))
    return out


def check(H, ints, records, value_of, nelec, doctor=None, want=None):
    """records: [(source, pqrs, new)]; value_of(k) -> the update's value for record k (a door's output, or None to take this
    module's update with `doctor`); want: brute_many of the new determinants, if the caller has it.
    Returns (failures, worst |delta| / bound)."""
    fails, worst = [], 0.0
    if want is None:
        want = brute_many(H, [r[2] for r in records])
    for k, (src, pqrs, new) in enumerate(records):
        old = brute(H, src)[0]
        ref, s_abs, _ = update(ints, H.norb, old, pqrs, new[0], new[1])
        got = value_of(k) if value_of else (ref if doctor is None else update(ints, H.norb, old, pqrs, new[0], new[1], doctor)[0])
        b = bound(old, s_abs, nelec)
        d = abs(got - float(want[k]))
        if not d <= b:
            fails.append((src, pqrs, got, float(want[k]), b))
        worst = max(worst, d / b)
    return fails, worst
