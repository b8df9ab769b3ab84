"""Plain-Python restatement of the reference's Cauchy-Schwarz proposal, written from the Fortran text of
chemistry.f90 (setup_orb_by_symm 2461-2527, off_diagonal_move_chem_cauchySchwarz 2530-4233), live branches
only (uniform_sampling is .false. after setup_orb_by_symm, 2526), time_sym = .false., no importance sampling.

The decisions of tests/golden/README_cauchyschwarz.md are built in:
  1. every intrinsic `call random_number` draw is taken from the move's own stream at the same position;
  2. a cumulative search that rounding leaves short of its draw is a null move (level 0, weight 0) with the
     draws taken so far consumed.

Three pieces: the tables (CSTables), the move (CSTables.move, one proposal from a stream), and the exact
path enumerator (CSTables.enumerate): every (level, e1, e2, hole1, hole2) path with its probability mass,
and for every reachable det_j the proposal probability the move reports for it.  rannyu / random_int are
48-bit integer arithmetic (rannyu.f90:54-74, tools.f90:129-147)."""
import math

import numpy as np

LCG_MULT = 34522712143931          # 11^13
MASK48 = (1 << 48) - 1
STOP_BELOW = float(np.float32(-1e-6))      # `integrals(int_index).lt.-1e-6`: a default-real literal (2514)


def seed_state(seed):
    """setrn: four 12-bit limbs, the last one made odd"""
    return ((seed[0] << 36) + (seed[1] << 24) + (seed[2] << 12) + 2 * (seed[3] // 2) + 1) & MASK48


def limbs_state(seed):
    """the four limbs as they stand (the test doors' seeds)"""
    return ((seed[0] << 36) + (seed[1] << 24) + (seed[2] << 12) + seed[3]) & MASK48


def state_limbs(x):
    return [(x >> 36) & 4095, (x >> 24) & 4095, (x >> 12) & 4095, x & 4095]


class Rannyu:
    """the reference's rannyu; draw() is rannyu(), rint(n) is random_int(n)"""

    def __init__(self, state):
        self.x = state & MASK48
        self.n = 0

    def draw(self):
        self.x = (self.x * LCG_MULT) & MASK48
        self.n += 1
        return self.x * 2.0 ** -48

    def rint(self, n):
        return int(n * self.draw()) + 1


class NegativeIntegrals(ValueError):
    pass


def _bits(x):
    """1-based orbitals of the set bits of x, ascending"""
    out, k = [], 1
    while x:
        if x & 1:
            out.append(k)
        x >>= 1; k += 1
    return out


class CSTables:
    """setup_orb_by_symm's Cauchy-Schwarz tables for one system and the move that uses them.

    orbsym: 1-based irreps of the orbitals (index 0 unused); prod: product_table, 1-based ([i][j]);
    integrals: the 1-based packed array; c2: combine_2 (1-based, [i][j]).  The integrals are clamped in place,
    as the reference does (2515)."""

    def __init__(self, norb, nup, ndn, ncore, orbsym, prod, integrals, c2):
        self.norb, self.nup, self.ndn, self.nc = norb, nup, ndn, ncore
        self.nelec = nup + ndn
        self.orbsym = [int(v) for v in orbsym]
        self.prod = [[int(v) for v in row] for row in np.asarray(prod).reshape(9, 9)]
        self.ngroup = max(self.orbsym[1:norb + 1])
        self.which = {s: [i for i in range(1, norb + 1) if self.orbsym[i] == s] for s in range(1, 9)}
        n = norb
        idx = lambda i, j: (lambda a: a * (a - 1) // 2 + a)(int(c2[i][j]))
        # the stop first: the reference stops at the first offender, and nothing it clamped before matters then
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                if integrals[idx(i, j)] < STOP_BELOW:
                    raise NegativeIntegrals("Negative integrals!")
        self.n_clamped = 0
        self.sq = [[0.0] * (n + 1) for _ in range(n + 1)]
        self.orb = [0.0] * (n + 1)
        self.sym = [[0.0] * (n + 1) for _ in range(9)]
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                s1 = self.orbsym[j]
                k = idx(i, j)
                if integrals[k] < 0:
                    integrals[k] = 0.0
                    self.n_clamped += 1
                self.sq[i][j] = math.sqrt(integrals[k])
                self.sym[s1][i] = self.sym[s1][i] + self.sq[i][j]
                self.orb[i] = self.orb[i] + self.sq[i][j]
        nc = ncore
        self.n_single = (nup - nc) * (norb - nup) + (ndn - nc) * (norb - ndn)
        self.n_double = ((nup - nc) * (nup - nc - 1) * (norb - nup) * (norb - nup - 1) // 4
                         + (ndn - nc) * (ndn - nc - 1) * (norb - ndn) * (norb - ndn - 1) // 4
                         + (nup - nc) * (norb - nup) * (ndn - nc) * (norb - ndn))
        self.n_total = self.n_single + self.n_double

    # ------------------------------------------------------------------ pieces of the move
    def _occ(self, iu, id_):
        """occ_orb: up ascending then dn ascending; the active range skips n_core_orb of each"""
        ou, od = _bits(iu), _bits(id_)
        assert len(ou) == self.nup and len(od) == self.ndn
        return ou, od

    def _prime_spin(self, o, ou, od):          # cs_sqrt_prime_spin (2721-2727)
        v = 2 * self.orb[o]
        for j in ou + od:
            v = v - self.sq[o][j]
        return v

    def _prime(self, o, own):                  # cs_sqrt_prime (2709-2720)
        v = self.orb[o]
        for j in own:
            v = v - self.sq[o][j]
        return v

    def _electrons(self, iu, id_):
        """the active electrons in occ_orb order as (orbital, is_up), their cs_sqrt_prime_spin, and sum_cs_sqrt_prime"""
        ou, od = self._occ(iu, id_)
        act = [(o, True) for o in ou[self.nc:]] + [(o, False) for o in od[self.nc:]]
        csp = [self._prime_spin(o, ou, od) for o, _ in act]
        s = 0.0
        for v in csp:
            s = s + v
        return ou, od, act, csp, s

    def _pair_sum(self, o1, o2, orbs):         # the electron_prob loops in front of a denominator
        acc = 0.0
        for x in orbs:
            acc = acc + self.sq[o2][x] + self.sq[o1][x]
        return acc

    @staticmethod
    def _pair_prob(c1, c2, s):                  # 2857-2860
        return c1 / s * c2 / (s - c1) + c2 / s * c1 / (s - c2)

    def _first_hole_list(self, iu, id_, up1, up2):
        """(orbital, is_up) of the first hole's candidates in the reference's scan order"""
        n = self.norb
        if up1 == up2:
            d = iu if up1 else id_
            return [(x, up1) for x in range(1, n + 1) if not (d >> (x - 1)) & 1]
        return [(x, True) for x in range(1, n + 1) if not (iu >> (x - 1)) & 1] + [(x, False) for x in range(1, n + 1) if not (id_ >> (x - 1)) & 1]

    def _den1(self, o1, o2, up1, up2, ou, od):
        if up1 == up2:
            own = ou if up1 else od
            return self._prime(o1, own) + self._prime(o2, own)
        return self._prime_spin(o1, ou, od) + self._prime_spin(o2, ou, od)

    def _second_hole(self, o1, o2, sym1, h1, h1up, same_spin, ou, od):
        """open orbitals of the second hole (ascending), its denominator; None when i_open = 0 (a return with weight 0)"""
        s1 = self.orbsym[h1]
        if same_spin:
            sym2 = self.prod[s1][sym1]
            occ = [x for x in (ou if h1up else od) if self.orbsym[x] == sym2]
            if sym2 == s1:
                occ = sorted(occ + [h1])
        else:
            sym2 = self.prod[sym1][s1]
            occ = [x for x in (od if h1up else ou) if self.orbsym[x] == sym2]
        opn = [x for x in self.which[sym2] if x not in occ]
        if not opn:
            return None
        den = self.sym[sym2][o2] + self.sym[sym2][o1] - self._pair_sum(o1, o2, occ)
        return opn, den, sym2

    def _temp_prob(self, o1, o2, h1, h1up, h2, den1, den, sym2, same_spin, ou, od):
        """temp_prob: both orders in which the two holes could have been drawn (3159-3188 / 3452-3481 / 3716-3743 / 3916-3943)"""
        sq = self.sq
        temp = (sq[o1][h1] + sq[o2][h1]) / den1 * (sq[o2][h2] + sq[o1][h2]) / den
        s1 = self.orbsym[h1]
        if same_spin:
            if sym2 == s1:
                den = den + sq[o2][h1] - sq[o2][h2] + sq[o1][h1] - sq[o1][h2]
            else:
                occ = [x for x in (ou if h1up else od) if self.orbsym[x] == s1]
                den = self.sym[s1][o2] + self.sym[s1][o1] - self._pair_sum(o1, o2, occ)
            return temp + (sq[o1][h2] + sq[o2][h2]) / den1 * (sq[o2][h1] + sq[o1][h1]) / den
        own1 = ou if h1up else od
        if len(self.which[s1]) - len([x for x in own1 if self.orbsym[x] == s1]) != 0:
            occ = [x for x in own1 if self.orbsym[x] == s1]
            den3 = self.sym[s1][o2] + self.sym[s1][o1] - self._pair_sum(o1, o2, occ)
            temp = temp + (sq[o1][h2] + sq[o2][h2]) / den1 * (sq[o2][h1] + sq[o1][h1]) / den3
        return temp

    def _search(self, weights, r):
        """index of the first cumulative sum >= r, or None (falls through)"""
        ep = 0.0
        for k, w in enumerate(weights):
            ep = ep + w
            if r <= ep:
                return k
        self.fell_through = True
        return None

    @staticmethod
    def _flip(iu, id_, o, up, on):
        b = 1 << (o - 1)
        if up:
            iu = (iu | b) if on else (iu & ~b)
        else:
            id_ = (id_ | b) if on else (id_ & ~b)
        return iu, id_

    def _singles(self, iu, id_, e):
        """the single excitation of active electron index e (1-based over up then dn): orbital, spin, open holes"""
        up = not (e > self.nup - self.nc)
        ou, od = self._occ(iu, id_)
        o = ou[e + self.nc - 1] if up else od[e + 2 * self.nc - self.nup - 1]
        own = iu if up else id_
        opn = [x for x in self.which[self.orbsym[o]] if not (own >> (x - 1)) & 1]
        return o, up, opn

    # ------------------------------------------------------------------ the move
    def move(self, iu, id_, rng):
        """one proposal; returns (level, det_j_up, det_j_dn, proposal_prob); level 0 = no move (det_j = det_i).
        self.fell_through tells whether the null move came from a cumulative search that fell through (decision 2)."""
        self.fell_through = False
        if rng.rint(self.n_total) <= self.n_single:
            prob = 1.0 * self.n_single / (self.n_total * 1.0)
            e = rng.rint(self.nelec - 2 * self.nc)
            o, up, opn = self._singles(iu, id_, e)
            prob = prob / (self.nelec - 2 * self.nc)
            if not opn:
                return 0, iu, id_, 0.0
            k = rng.rint(len(opn))
            prob = prob / len(opn)
            ju, jd = self._flip(iu, id_, o, up, False)
            ju, jd = self._flip(ju, jd, opn[k - 1], up, True)
            return 1, ju, jd, prob
        prob = self.n_double / float(self.n_total)
        ou, od, act, csp, s = self._electrons(iu, id_)
        k1 = self._search([v / s for v in csp], rng.draw())
        if k1 is None:
            return 0, iu, id_, 0.0
        rest = [k for k in range(len(act)) if k != k1]
        k2 = self._search([csp[k] / (s - csp[k1]) for k in rest], rng.draw())
        if k2 is None:
            return 0, iu, id_, 0.0
        k2 = rest[k2]
        prob = prob * self._pair_prob(csp[k1], csp[k2], s)
        r = self._double_holes(iu, id_, ou, od, act, min(k1, k2), max(k1, k2), rng)
        if r is None:
            return 0, iu, id_, 0.0
        ju, jd, temp = r
        return 2, ju, jd, prob * temp

    def _double_holes(self, iu, id_, ou, od, act, ka, kb, rng):
        (o1, up1), (o2, up2) = act[ka], act[kb]
        same = up1 == up2
        sym1 = self.prod[self.orbsym[o1]][self.orbsym[o2]]
        den1 = self._den1(o1, o2, up1, up2, ou, od)
        cand = self._first_hole_list(iu, id_, up1, up2)
        k = self._search([(self.sq[o1][x] + self.sq[o2][x]) / den1 for x, _ in cand], rng.draw())
        if k is None:
            return None
        h1, h1up = cand[k]
        sh = self._second_hole(o1, o2, sym1, h1, h1up, same, ou, od)
        if sh is None:
            return None
        opn, den, sym2 = sh
        k = self._search([(self.sq[o2][x] + self.sq[o1][x]) / den for x in opn], rng.draw())
        if k is None:
            return None
        h2 = opn[k]
        ju, jd = self._flip(iu, id_, o1, up1, False)
        ju, jd = self._flip(ju, jd, o2, up2, False)
        ju, jd = self._flip(ju, jd, h1, h1up, True)
        ju, jd = self._flip(ju, jd, h2, h1up if same else not h1up, True)
        return ju, jd, self._temp_prob(o1, o2, h1, h1up, h2, den1, den, sym2, same, ou, od)

    # ------------------------------------------------------------------ the exact path enumerator
    def enumerate(self, iu, id_):
        """every path of the move from (iu, id_) with its probability mass (exact weights, no draw granularity).
        Returns (paths, null_mass, reported): paths = list of (level, e1, e2, hole1, hole2, det_j, mass), electrons
        and holes as (orbital, is_up); null_mass = the mass of the returns with weight 0; reported[det_j] = the
        proposal probability the move reports for det_j (one value per det_j, checked to be path-independent)."""
        paths, null, reported = [], 0.0, {}

        def report(dj, p):
            if dj in reported:
                assert abs(reported[dj] - p) <= 1e-12 * max(1.0, abs(p)), (dj, reported[dj], p)
            else:
                reported[dj] = p

        ne = self.nelec - 2 * self.nc
        p_single = self.n_single / self.n_total
        p_double = self.n_double / self.n_total
        for e in range(1, ne + 1):
            o, up, opn = self._singles(iu, id_, e)
            if not opn:
                null += p_single / ne
                continue
            for h in opn:
                ju, jd = self._flip(iu, id_, o, up, False)
                ju, jd = self._flip(ju, jd, h, up, True)
                paths.append((1, (o, up), None, (h, up), None, (ju, jd), p_single / ne / len(opn)))
                report((ju, jd), 1.0 * self.n_single / (self.n_total * 1.0) / ne / len(opn))
        ou, od, act, csp, s = self._electrons(iu, id_)
        for k1 in range(len(act)):
            for k2 in range(len(act)):
                if k2 == k1:
                    continue
                pe = csp[k1] / s * (csp[k2] / (s - csp[k1]))
                ka, kb = min(k1, k2), max(k1, k2)
                (o1, up1), (o2, up2) = act[ka], act[kb]
                same = up1 == up2
                sym1 = self.prod[self.orbsym[o1]][self.orbsym[o2]]
                den1 = self._den1(o1, o2, up1, up2, ou, od)
                for h1, h1up in self._first_hole_list(iu, id_, up1, up2):
                    p1 = (self.sq[o1][h1] + self.sq[o2][h1]) / den1
                    sh = self._second_hole(o1, o2, sym1, h1, h1up, same, ou, od)
                    if sh is None:
                        null += p_double * pe * p1
                        continue
                    opn, den, sym2 = sh
                    for h2 in opn:
                        p2 = (self.sq[o2][h2] + self.sq[o1][h2]) / den
                        ju, jd = self._flip(iu, id_, o1, up1, False)
                        ju, jd = self._flip(ju, jd, o2, up2, False)
                        ju, jd = self._flip(ju, jd, h1, h1up, True)
                        ju, jd = self._flip(ju, jd, h2, h1up if same else not h1up, True)
                        paths.append((2, act[k1], act[k2], (h1, h1up), (h2, h1up if same else not h1up), (ju, jd), p_double * pe * p1 * p2))
                        temp = self._temp_prob(o1, o2, h1, h1up, h2, den1, den, sym2, same, ou, od)
                        report((ju, jd), self.n_double / float(self.n_total) * self._pair_prob(csp[k1], csp[k2], s) * temp)
        return paths, null, reported


def from_host(host):
    """CSTables of a ChemHost (its parsed FCIDUMP: orbital irreps, product table, integrals, combine_2), on a copy of the integrals"""
    return CSTables(host.norb, host.nup, host.ndn, host.n_core_orb, list(host.orbsym), np.asarray(host.prod), np.array(host.integrals, copy=True),
                    np.asarray(host.combine_2))
