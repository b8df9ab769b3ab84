"""An independent model of the zeroth-order Green's function of a determinant expansion
(get_zeroth_order_variational_greens_function, hci.f90:3849-4050).  Nothing here comes from sqmc_amd/ or oracle/: it loops over all
determinants, all (q, sigma) and all p, applies a+ and a to occupation tuples (tests/rdm_checker.py), looks determinants up in a dict,
and takes H_mm from tests/proposal_checker.py, whose Hamiltonian acts on Fock-space bit strings of any electron number.

  G_np1(w, p, q) = sum_sigma sum_i c_i c_k s / (w - (H_mm - e0)),   a+_{q sigma} |i> = s1 |m>,  a_{p sigma} |m> = s2 |k>
  G_nm1(w, p, q) = sum_sigma sum_i c_i c_k s / (w - (e0 - H_mm)),   a_{q sigma} |i> = s1 |m>,   a+_{p sigma} |m> = s2 |k>
k in the list.  s = s1 s2 in the signed mode (the matrix elements <a_p (w - (H0 - E0))^-1 a+_q> and <a+_p (w - (E0 - H0))^-1 a_q> of the
reference's header comment) and s = 1 in the unsigned mode (what the reference's loops compute: no fermionic sign).  A determinant
is the up string's operators in ascending order followed by the dn string's (rdm_checker's convention): an operator of the dn string
passes all nup up operators, a+_q and a_p (or a_q and a+_p) both do and nup does not change in between, so those factors cancel and the
sign is that of the two operators on the sigma tuple alone.

Bound on |kernel - checker| of an entry with n terms t_j = A_j / (w - x_j), A_j = the rounded product c_i c_k (the same double in the
kernel: the product commutes and the sign is exact):
  (n + 3) 2^-53 sum|t_j|       the n - 1 additions in any order, the quotient, the subtraction w - x in the denominator (relative to
                               the term it is at most 2^-53 |w - x| / |w - x|), the checker's own fsum, and one to spare for the
                               product being compared through a quotient
  + sum_j |A_j| delta_j / (d_j (d_j - delta_j))        d_j = |w - x_j| here, delta_j = the bound on the difference of the two
                               denominators = rounding_bound(n_H, sum|H terms|) of H_mm + 2^-53 (|H_mm| + |e0| + |w|) for the roundings
                               of x = H_mm - e0 and of w - x on both sides.
The checker asserts d_j > 2 delta_j for every term it evaluates, and compare() asserts that every bound is below 1e-8 of the entry's
sum|t_j|: a case that cannot meet this is an error in the test's construction, not something to skip."""
import math

from tests import proposal_checker as PC
from tests import rdm_checker as RC

U = 2.0 ** -53
NP1, NM1 = "np1", "nm1"
REL_BOUND_MAX = 1e-8
D_MIN = 0.05


def _string(occ):
    return sum(1 << k for k in occ)


class Entry:
    """one (part, p, q) at one frequency, in both sign modes"""
    __slots__ = ("n", "unsigned", "signed", "sum_abs", "bound")

    def __init__(self, n, unsigned, signed, sum_abs, bound):
        self.n, self.unsigned, self.signed, self.sum_abs, self.bound = n, unsigned, signed, sum_abs, bound

    def value(self, signed):
        return self.signed if signed else self.unsigned


class Greens:
    """terms[part][(p, q)] = [(A, sign, x, H_mm, bound on H_mm)]; H: a proposal_checker Hamiltonian; dets: [(up, dn)] integers"""
    _hmm = {}                # (id(H), up, dn) -> element(): the diagonal of an N+-1 electron determinant, kept across instances

    def __init__(self, H, dets, coeffs, e0, norb):
        dets = [(int(a), int(b)) for a, b in dets]
        assert len(set(dets)) == len(dets), "a determinant appears twice"
        self.H, self.norb, self.e0 = H, norb, float(e0)
        self.c = [float(x) for x in coeffs]
        occ = [(RC.occupation(a), RC.occupation(b)) for a, b in dets]
        where = {o: k for k, o in enumerate(occ)}
        self.terms = {NP1: {}, NM1: {}}
        for i, (ui, di) in enumerate(occ):
            for sigma in (0, 1):
                s = di if sigma else ui
                for q in range(norb):
                    for part, first, second in ((NP1, RC.create, RC.annihilate), (NM1, RC.annihilate, RC.create)):
                        got = first(s, q)
                        if got is None:
                            continue
                        m, s1 = got
                        mu, md = (_string(ui), _string(m)) if sigma else (_string(m), _string(di))
                        hmm = None
                        for p in range(norb):
                            back = second(m, p)
                            if back is None:
                                continue
                            ks, s2 = back
                            k = where.get((ui, ks) if sigma else (ks, di))
                            if k is None:
                                continue
                            if hmm is None:
                                hmm = self.diagonal(mu, md)
                            x = (hmm[0] - self.e0) if part == NP1 else (self.e0 - hmm[0])
                            self.terms[part].setdefault((p, q), []).append((self.c[i] * self.c[k], s1 * s2, x, hmm[0], PC.rounding_bound(hmm[1], hmm[2])))

    def diagonal(self, mu, md):
        key = (id(self.H), mu, md)
        if key not in Greens._hmm:
            Greens._hmm[key] = self.H.element(mu, md, mu, md)
        return Greens._hmm[key]

    def count(self, part, p, q):
        return len(self.terms[part].get((p, q), ()))

    def poles(self, part):
        """every x of the part's terms, sorted, repeats removed"""
        return sorted(set(t[2] for lst in self.terms[part].values() for t in lst))

    def all_poles(self):
        return sorted(set(self.poles(NP1)) | set(self.poles(NM1)))

    def max_h_bound(self):
        return max(t[4] for part in (NP1, NM1) for lst in self.terms[part].values() for t in lst)

    def entry(self, part, p, q, w):
        lst = self.terms[part].get((p, q), ())
        w = float(w)
        un, sg, amp = [], [], 0.0
        for a, sign, x, hmm, hb in lst:
            den = w - x
            d = abs(den)
            delta = hb + U * (abs(hmm) + abs(self.e0) + abs(w))
            assert d > 2.0 * delta, "a frequency within rounding of a pole: w = %r, x = %r" % (w, x)
            t = a / den
            un.append(t); sg.append(sign * t)
            amp += abs(a) * delta / (d * (d - delta))
        sa = math.fsum(abs(t) for t in un)
        return Entry(len(lst), math.fsum(un), math.fsum(sg), sa, (len(lst) + 3) * U * sa + amp)

    def residues(self, part):
        """signed mode with every residue summed: {(p, q): (sum of sign A, n, sum |A|)}"""
        return {pq: (math.fsum(t[1] * t[0] for t in lst), len(lst), math.fsum(abs(t[0]) for t in lst)) for pq, lst in self.terms[part].items()}

    def sum_rule_bound(self, part, p, q, w):
        """bound on |w G(w, p, q) - R(p, q)| for the kernel's G at a frequency far outside the poles (|w| a power of two, so w G is
        exact): w A / (w - x) - A = A x / (w - x), at most |A| max|x| / (|w| - max|x|) per term, plus |w| times the entry's bound"""
        lst = self.terms[part].get((p, q), ())
        if not lst:
            return 0.0
        xm = max(abs(t[2]) for t in lst)
        assert abs(w) > 2.0 * xm
        return math.fsum(abs(t[0]) for t in lst) * xm / (abs(w) - xm) + abs(w) * self.entry(part, p, q, w).bound

    def compare(self, part, signed, w, got):
        """got[i_w][p][q] against the model at the frequencies w: ([(i_w, p, q, got, expected, bound)] of the entries out of bound,
        worst |delta| / bound).  Entries without a term must be exactly 0.0"""
        fails, worst = [], 0.0
        for i_w, ww in enumerate(w):
            for p in range(self.norb):
                for q in range(self.norb):
                    v = float(got[i_w][p][q])
                    if not self.count(part, p, q):
                        if not (v == 0.0):
                            fails.append((i_w, p, q, v, 0.0, 0.0))
                        continue
                    e = self.entry(part, p, q, ww)
                    assert e.bound < REL_BOUND_MAX * e.sum_abs, "the case is badly built: bound %r against sum|terms| %r at w = %r" % (e.bound, e.sum_abs, ww)
                    delta = abs(v - e.value(signed))
                    if not delta <= e.bound:
                        fails.append((i_w, p, q, v, e.value(signed), e.bound))
                    if e.bound > 0.0:
                        worst = max(worst, delta / e.bound)
        return fails, worst


def rayleigh_quotient(H, dets, coeffs):
    """<psi|H|psi> / <psi|psi> over all pairs of a short list"""
    num = []
    for (iu, id_), ci in zip(dets, coeffs):
        for (ju, jd), cj in zip(dets, coeffs):
            v = H.element(int(iu), int(id_), int(ju), int(jd))[0]
            if v != 0.0:
                num.append(ci * cj * v)
    return math.fsum(num) / math.fsum(c * c for c in coeffs)


# ---------------------------------------------------------------------------------------------- frequencies, from the pole list alone
def outside(poles, margin=1.0):
    """one point below the lowest and one above the highest pole"""
    return [min(poles) - margin, max(poles) + margin]


def wide_gaps(poles, d_min=D_MIN):
    """how many interior gaps have room for a midpoint d_min from both ends"""
    ps = sorted(set(poles))
    return sum(1 for a, b in zip(ps, ps[1:]) if 0.5 * (a + b) - a >= d_min and b - 0.5 * (a + b) >= d_min)


def in_gaps(poles, k, d_min=D_MIN):
    """midpoints of the k largest interior gaps, each at least d_min from every pole"""
    ps = sorted(set(poles))
    gaps = sorted(((b - a, 0.5 * (a + b)) for a, b in zip(ps, ps[1:])), reverse=True)[:k]
    assert len(gaps) == k, "fewer than %d interior gaps" % k
    out = [mid for _, mid in gaps]
    for wv in out:
        assert min(abs(wv - x) for x in ps) >= d_min, "a gap midpoint %r closer than %r to a pole" % (wv, d_min)
    return out


def uniform(poles, n_w, d_min=D_MIN):
    """(w_min, w_max) of a uniform grid of n_w points (w_min + (w_max - w_min) i / (n_w - 1)) every point of which is at least d_min
    from every pole: the first of a fixed sequence of windows around the pole list that has the property"""
    ps = sorted(set(poles))
    lo, hi = min(ps), max(ps)
    for k in range(2000):
        w_min, w_max = lo - 0.3 - 0.0137 * k, hi + 0.3 + 0.0071 * k
        grid = [w_min + (w_max - w_min) * i / (n_w - 1.0) for i in range(n_w)]
        if all(min(abs(wv - x) for x in ps) >= d_min for wv in grid):
            return w_min, w_max
    raise AssertionError("no uniform grid of %d points keeps %r from every pole" % (n_w, d_min))
