"""An independent brute force for the two-body reduced density matrix of a determinant expansion, in the three spin blocks of
sqmc_gpu_hci_2rdm.  Nothing here comes from sqmc_amd/ or oracle/: for every ordered pair of determinants of the list the four
operators are applied one after the other to occupation tuples (tests/rdm_checker.py's annihilate / create); no intermediates, no
ranks, no sorting.

Convention (0-based): a determinant is the tuple of its occupied spin orbitals in ascending order, spin orbital P = p for an up
electron in orbital p and norb + p for a dn electron -- all up operators in front of all dn operators, as tests/proposal_checker.py.
  aa[p,q,r,s] = <a+_{p up} a+_{q up} a_{s up} a_{r up}>,  bb the same with dn,  ab[p,q,r,s] = <a+_{p up} a+_{q dn} a_{s dn} a_{r up}>
A term of an entry is sign c_i c_j with a+_P a+_Q a_S a_R |j> = sign |i> (a_R acts first).  Per entry the terms are kept, so that
value = fsum(terms), n = their number, s = sum |term|; the bound on |kernel - checker| is proposal_checker.rounding_bound(n, s):
the kernel's terms are the same doubles (a sign is exact, the product c_i c_j is rounded once and commutes) and a double-precision
sum of n terms in any order stays within (n - 1) 2^-53 s of the exact one.

Also here, from first principles: <S^2> through S_+ applied to the determinants, and the energy through proposal_checker's t / v."""
import math
from itertools import combinations

from tests import proposal_checker as PC
from tests import rdm_checker as RC

BLOCKS = ("aa", "bb", "ab")


def spin_orbitals(up, dn, norb):
    return RC.occupation(up) + tuple(norb + q for q in RC.occupation(dn))


def block_of(P, Q, R, S, norb):
    """the stored block of a+_P a+_Q a_S a_R and its orbital indices, or None (the dn-up order is not stored)"""
    sp = (P >= norb, Q >= norb, R >= norb, S >= norb)
    idx = (P % norb, Q % norb, R % norb, S % norb)
    if sp == (False, False, False, False):
        return "aa", idx
    if sp == (True, True, True, True):
        return "bb", idx
    if sp == (False, True, False, True):
        return "ab", idx
    return None


def apply_string(occ, P, Q, R, S):
    """a+_P a+_Q a_S a_R on an occupation tuple: (tuple, sign) or None"""
    sign, cur = 1, occ
    for op, X in ((RC.annihilate, R), (RC.annihilate, S), (RC.create, Q), (RC.create, P)):
        got = op(cur, X)
        if got is None:
            return None
        cur, sign = got[0], sign * got[1]
    return cur, sign


def operator_strings(occ_i, occ_j):
    """every (P, Q, R, S) with a+_P a+_Q a_S a_R |j> = +-|i>, for two determinants at most two spin orbitals apart"""
    si, sj = set(occ_i), set(occ_j)
    gone, come = sj - si, si - sj
    if len(gone) > 2 or len(gone) != len(come):
        return
    common = sorted(sj & si)
    for extra in combinations(common, 2 - len(gone)):
        A, B = sorted(gone | set(extra)), sorted(come | set(extra))
        for R, S in ((A[0], A[1]), (A[1], A[0])):
            for P, Q in ((B[0], B[1]), (B[1], B[0])):
                yield P, Q, R, S


class Rdm2:
    def __init__(self, norb):
        self.norb = norb
        self.terms = {b: {} for b in BLOCKS}
        self.reached = {b: set() for b in BLOCKS}      # every entry some pair of determinants reaches, sampled or not

    def value(self, b, idx):
        return math.fsum(self.terms[b].get(idx, ()))

    def count(self, b, idx):
        return len(self.terms[b].get(idx, ()))

    def sum_abs(self, b, idx):
        return math.fsum(abs(x) for x in self.terms[b].get(idx, ()))

    def bound(self, b, idx):
        return PC.rounding_bound(self.count(b, idx), self.sum_abs(b, idx))

    def spin_free(self, idx):
        """(value, bound) of G[p,q,r,s] = aa + bb + ab[p,q,r,s] + ab[q,p,s,r]"""
        p, q, r, s = idx
        parts = [("aa", idx), ("bb", idx), ("ab", idx), ("ab", (q, p, s, r))]
        return math.fsum(self.value(b, k) for b, k in parts), math.fsum(self.bound(b, k) for b, k in parts) + 4 * RC.U * math.fsum(abs(self.value(b, k)) for b, k in parts)


def _close_pairs(states):
    """ordered pairs (i, j) of determinants at most two spin orbitals apart (a larger distance has no term)"""
    n = len(states)
    for i in range(n):
        si = states[i]
        for j in range(n):
            if bin(si ^ states[j]).count("1") <= 4:
                yield i, j


def two_rdm(dets, coeffs, norb, sample=None):
    """dets: [(up, dn)] as integers, coeffs: floats.  sample: {block: set of (p, q, r, s)}; given, only those entries are formed"""
    dets = [(int(a), int(b)) for a, b in dets]
    assert len(set(dets)) == len(dets), "a determinant appears twice"
    occ = [spin_orbitals(a, b, norb) for a, b in dets]
    states = [a | (b << norb) for a, b in dets]
    c = [float(x) for x in coeffs]
    out = Rdm2(norb)
    for i, j in _close_pairs(states):
        for P, Q, R, S in operator_strings(occ[i], occ[j]):
            where = block_of(P, Q, R, S, norb)
            if where is None:
                continue
            out.reached[where[0]].add(where[1])
            if sample is not None and where[1] not in sample[where[0]]:
                continue
            got = apply_string(occ[j], P, Q, R, S)
            assert got is not None and got[0] == occ[i]
            out.terms[where[0]].setdefault(where[1], []).append(got[1] * (c[i] * c[j]))
    return out


def pattern(dets, norb):
    """{block: set of entries that some pair of determinants reaches}: the cheap pass, no signs and no values"""
    dets = [(int(a), int(b)) for a, b in dets]
    occ = [spin_orbitals(a, b, norb) for a, b in dets]
    states = [a | (b << norb) for a, b in dets]
    out = {b: set() for b in BLOCKS}
    for i, j in _close_pairs(states):
        for P, Q, R, S in operator_strings(occ[i], occ[j]):
            where = block_of(P, Q, R, S, norb)
            if where is not None:
                out[where[0]].add(where[1])
    return out


def compare(exp, got, blocks=BLOCKS, sample=None):
    """got: {block: array indexed [p, q, r, s]} against an Rdm2: (failures, worst |delta| / bound, entries compared).  With a sample
    only its entries are looked at; without one every entry of the arrays is, and one without terms must be exactly 0.0"""
    import numpy as np
    fails, worst, seen = [], 0.0, 0
    for b in blocks:
        a = got[b]
        keys = sample[b] if sample is not None else set(exp.terms[b]) | set(map(tuple, np.argwhere(a != 0.0).tolist()))
        for idx in keys:
            x, want, bd = float(a[idx]), exp.value(b, idx), exp.bound(b, idx)
            seen += 1
            if exp.count(b, idx) == 0 or bd == 0.0:
                if x != want:
                    fails.append((b, idx, x, want, 0.0))
                continue
            d = abs(x - want)
            if not d <= bd:
                fails.append((b, idx, x, want, bd))
            worst = max(worst, d / bd)
    return fails, worst, seen


def norm2(coeffs):
    return math.fsum(float(x) * float(x) for x in coeffs)


def s_squared(dets, coeffs, norb):
    """<Psi| S^2 |Psi> = |S_+ Psi|^2 + (Sz^2 + Sz) <Psi|Psi>, S_+ = sum_p a+_{p up} a_{p dn} applied to the occupation tuples"""
    dets = [(int(a), int(b)) for a, b in dets]
    raised = {}
    for (a, b), ci in zip(dets, coeffs):
        occ = spin_orbitals(a, b, norb)
        for p in range(norb):
            got = RC.annihilate(occ, norb + p)
            if got is None:
                continue
            got2 = RC.create(got[0], p)
            if got2 is None:
                continue
            raised.setdefault(got2[0], []).append(got[1] * got2[1] * float(ci))
    nup, ndn = len(RC.occupation(dets[0][0])), len(RC.occupation(dets[0][1]))
    sz = 0.5 * (nup - ndn)
    sq = [math.fsum(v) ** 2 for v in raised.values()]
    return math.fsum(sq + [(sz * sz + sz) * norm2(coeffs)])


def s_squared_bound(dets, coeffs, norb, two=None):
    """bound on |formula - s_squared| for <S^2> formed as (Sz^2 + Sz + ndn) sum c^2 - sum_pq ab[q,p,p,q] from matrices whose entries
    lie within `two`'s entry bounds (an Rdm2; None: exact entries).  In exact arithmetic on the doubles c_i the two agree.  s_squared
    squares a sum v of signed coefficients per raised determinant where the matrices hold the products c_i c_j one by one: every
    product is rounded once (2^-53 |c_i c_j|, together 2^-53 (sum |v|)^2), the square and the fsum in front of it twice more, the outer
    sums once each; the constant's three roundings and those of norm2 ride on (Sz^2 + Sz + ndn) sum c^2."""
    dets = [(int(a), int(b)) for a, b in dets]
    mass = {}
    for (a, b), ci in zip(dets, coeffs):
        occ = spin_orbitals(a, b, norb)
        for p in range(norb):
            got = RC.annihilate(occ, norb + p)
            got2 = RC.create(got[0], p) if got is not None else None
            if got2 is not None:
                mass[got2[0]] = mass.get(got2[0], 0.0) + abs(float(ci))
    nup, ndn = len(RC.occupation(dets[0][0])), len(RC.occupation(dets[0][1]))
    sz = 0.5 * (nup - ndn)
    sq = math.fsum(m * m for m in mass.values())
    const = (abs(sz * sz + sz) + ndn) * norm2(coeffs)
    out = 4 * RC.U * sq + 2 * RC.U * sq + 6 * RC.U * const
    if two is not None:
        ex = [(q, p, p, q) for p in range(norb) for q in range(norb)]
        out += math.fsum(two.bound("ab", k) for k in ex) + 2 * RC.U * math.fsum(abs(two.value("ab", k)) for k in ex)
    return out


def expectation(H, dets, coeffs):
    """(sum_ij c_i c_j <i|H|j>, bound, sum_ij |c_i c_j <i|H|j>|): every pair, H.element's own term counts propagated"""
    dets = [(int(a), int(b)) for a, b in dets]
    vals, bds = [], []
    for (iu, id_), ci in zip(dets, coeffs):
        for (ju, jd), cj in zip(dets, coeffs):
            h, n, s = H.element(ju, jd, iu, id_)
            if n:
                w = float(ci) * float(cj)
                vals.append(w * h)
                bds.append(abs(w) * (PC.rounding_bound(n, s) + 2 * RC.U * abs(h)))
    sa = math.fsum(abs(x) for x in vals)
    return math.fsum(vals), math.fsum(bds) + RC.U * sa, sa


def energy(H, one, two, n2):
    """(E, bound) = sum_pr t(p,r) D[p][r] + 1/2 sum (pr|qs) G[p,q,r,s] + const n2 from the checker's own matrices (one: an
    rdm_checker.Rdm, two: an Rdm2, n2 = sum c^2), t and v from proposal_checker"""
    norb = two.norb
    vals, bds = [H.const * n2], [2 * RC.U * abs(H.const * n2)]
    for p in range(norb):
        for r in range(norb):
            if one.count(p, r):
                t = H.t(p, r)
                vals.append(t * one.value(p, r)); bds.append(abs(t) * (one.bound(p, r) + 2 * RC.U * abs(one.value(p, r))))
    for b in BLOCKS:
        for (p, q, r, s) in two.terms[b]:
            # aa and bb enter once each; ab stands for both mixed orders, ab[p,q,r,s] and its image [q,p,s,r] with (qs|pr) = (pr|qs)
            v = H.v(p, r, q, s) * (1.0 if b == "ab" else 0.5)
            g = two.value(b, (p, q, r, s))
            vals.append(v * g); bds.append(abs(v) * (two.bound(b, (p, q, r, s)) + 2 * RC.U * abs(g)))
    return math.fsum(vals), math.fsum(bds) + RC.U * math.fsum(abs(x) for x in vals)


def partial_trace(two, p, r, nelec):
    """(sum_q G[p,q,r,q], bound), G the spin-free matrix"""
    got = [two.spin_free((p, q, r, q)) for q in range(two.norb)]
    return math.fsum(x for x, _ in got), math.fsum(b for _, b in got) + two.norb * RC.U * math.fsum(abs(x) for x, _ in got)
