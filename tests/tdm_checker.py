"""An independent brute force for the one- and two-body transition density matrices of two coefficient vectors, bra and ket, over one
determinant list, in the conventions of sqmc_gpu_hci_1tdm / sqmc_gpu_hci_2tdm (tests/golden/README_transition_rdm.md).  Nothing here
comes from sqmc_amd/ or oracle/: it is tests/rdm2_checker.py's loop over ordered pairs of determinants with the operators applied to
occupation tuples, and tests/rdm_checker.py's move for the one-body matrix; no intermediates, no ranks, no sorting.

  aa[p,q,r,s] = <bra| a+_{p up} a+_{q up} a_{s up} a_{r up} |ket>,  bb the same with dn,  ab[p,q,r,s] = <bra| a+_{p up} a+_{q dn} a_{s dn} a_{r up} |ket>
A term of a two-body entry is sign bra_i ket_j with a+_P a+_Q a_S a_R |j> = sign |i>.
  one[p][r] = <bra| a+_r a_p |ket> summed over spin: a term is sign ket_i bra_k with a+_{r sigma} a_{p sigma} |i> = sign |k>.
Per entry the terms are kept (an rdm2_checker.Rdm2 / rdm_checker.Rdm), so the bound on |kernel - checker| is
proposal_checker.rounding_bound(n, s) for a two-body entry and Rdm.bound for a one-body one: the kernel's terms are the same doubles
(a sign is exact, one rounded product that commutes) and a double-precision sum of n terms in any order stays within (n - 1) 2^-53 s
of the exact one.  Nothing is renormalised."""
import math

from tests import proposal_checker as PC
from tests import rdm_checker as RC
from tests import rdm2_checker as R2

BLOCKS = R2.BLOCKS


def two_tdm(dets, bra, ket, norb, sample=None, number=float):
    """dets: [(up, dn)] as integers.  sample: {block: container of (p, q, r, s)}; given, only those entries are formed (reached still
    holds every entry some pair of determinants reaches).  number: the type the terms are formed in (float, or fractions.Fraction)"""
    dets = [(int(a), int(b)) for a, b in dets]
    assert len(set(dets)) == len(dets), "a determinant appears twice"
    occ = [R2.spin_orbitals(a, b, norb) for a, b in dets]
    states = [a | (b << norb) for a, b in dets]
    u, w = [number(x) for x in bra], [number(x) for x in ket]
    out = R2.Rdm2(norb)
    for i, j in R2._close_pairs(states):
        for P, Q, R, S in R2.operator_strings(occ[i], occ[j]):
            where = R2.block_of(P, Q, R, S, norb)
            if where is None:
                continue
            out.reached[where[0]].add(where[1])
            if sample is not None and where[1] not in sample[where[0]]:
                continue
            got = R2.apply_string(occ[j], P, Q, R, S)
            assert got is not None and got[0] == occ[i]
            out.terms[where[0]].setdefault(where[1], []).append(got[1] * (u[i] * w[j]))
    return out


def one_tdm(dets, bra, ket, norb, orbital_symmetries=None, number=float):
    """all single moves of every determinant of the list, looked up by occupation tuples"""
    dets = [(int(a), int(b)) for a, b in dets]
    assert len(set(dets)) == len(dets), "a determinant appears twice"
    occ = [(RC.occupation(a), RC.occupation(b)) for a, b in dets]
    where = {o: k for k, o in enumerate(occ)}
    u, w = [number(x) for x in bra], [number(x) for x in ket]
    out = RC.Rdm(norb)
    same = (lambda p, r: True) if orbital_symmetries is None else (lambda p, r: orbital_symmetries[p] == orbital_symmetries[r])
    for i, (ui, di) in enumerate(occ):
        for spin, sigma in enumerate((ui, di)):
            for p in sigma:
                for r in range(norb):
                    got = RC.move(sigma, p, r)
                    if got is None or not same(p, r):
                        continue
                    k = where.get((got[0], di) if spin == 0 else (ui, got[0]))
                    if k is not None:
                        out.terms[p][r].append(got[1] * w[i] * u[k])
    return out


def overlap(bra, ket):
    return math.fsum(float(a) * float(b) for a, b in zip(bra, ket))


def expectation(H, dets, bra, ket):
    """(sum_ij bra_i ket_j <i|H|j>, bound, sum |terms|): rdm2_checker.expectation with two vectors"""
    dets = [(int(a), int(b)) for a, b in dets]
    vals, bds = [], []
    for (iu, id_), bi in zip(dets, bra):
        for (ju, jd), kj in zip(dets, ket):
            h, n, s = H.element(ju, jd, iu, id_)
            if n:
                w = float(bi) * float(kj)
                vals.append(w * h)
                bds.append(abs(w) * (PC.rounding_bound(n, s) + 2 * RC.U * abs(h)))
    sa = math.fsum(abs(x) for x in vals)
    return math.fsum(vals), math.fsum(bds) + RC.U * sa, sa


def energy(H, one, two, ovl):
    """(<bra|H|ket>, bound) from the checker's own transition matrices: rdm2_checker.energy with the overlap for sum c^2.  one is
    indexed [p][r] = <a+_r a_p>, and t is symmetric, so the one-body sum reads as there"""
    return R2.energy(H, one, two, ovl)


def s_squared_polarised(dets, bra, ket, norb):
    """<bra| S^2 |ket> = [<b+k| S^2 |b+k> - <b-k| S^2 |b-k>] / 4 from rdm2_checker.s_squared (S^2 is symmetric)"""
    plus = [float(a) + float(b) for a, b in zip(bra, ket)]
    minus = [float(a) - float(b) for a, b in zip(bra, ket)]
    return (R2.s_squared(dets, plus, norb) - R2.s_squared(dets, minus, norb)) / 4.0


def s_squared_polarised_bound(dets, bra, ket, norb):
    """bound on |exact <bra|S^2|ket> on the doubles bra, ket - s_squared_polarised|: rdm2_checker.s_squared against its own formula
    on exact entries (s_squared_bound) for both vectors, the roundings of bra +- ket (one per coefficient: the quadratic form moves by
    at most 3 2^-53 |S^2| |x|^2, |S^2| <= N/2 (N/2 + 1)) and the three roundings of the difference and the quarter"""
    plus = [float(a) + float(b) for a, b in zip(bra, ket)]
    minus = [float(a) - float(b) for a, b in zip(bra, ket)]
    n = len(RC.occupation(dets[0][0])) + len(RC.occupation(dets[0][1]))
    smax = 0.5 * n * (0.5 * n + 1.0)
    sp, sm = R2.s_squared(dets, plus, norb), R2.s_squared(dets, minus, norb)
    out = (R2.s_squared_bound(dets, plus, norb) + R2.s_squared_bound(dets, minus, norb)) / 4
    out += 3 * RC.U * smax * (R2.norm2(plus) + R2.norm2(minus)) / 4
    return out + 3 * RC.U * (abs(sp) + abs(sm)) / 4


def s_squared(two, dets, ovl):
    """<bra| S^2 |ket> = (Sz^2 + Sz + ndn) <bra|ket> - sum_pq ab[q,p,p,q] from an Rdm2 of transition terms, and the bound of the sum"""
    nup, ndn = len(RC.occupation(dets[0][0])), len(RC.occupation(dets[0][1]))
    sz = 0.5 * (nup - ndn)
    ex = [(q, p, p, q) for p in range(two.norb) for q in range(two.norb)]
    vals = [(sz * sz + sz + ndn) * ovl] + [-two.value("ab", k) for k in ex]
    return math.fsum(vals), math.fsum(two.bound("ab", k) for k in ex) + (len(ex) + 4) * RC.U * math.fsum(abs(x) for x in vals)
