"""Plain-Python restatement of the Cauchy-Schwarz proposal with time-reversal symmetry (time_sym = .true.), on top of
tests/cauchy_checker.py.  Written from the Fortran text of chemistry.f90:

  * the Cauchy-Schwarz arm of is_connected_chem (2203-2450; singles take the uniform formula, 2131-2152), literally
    (`literal_arm`, which may be handed the move tables of another parent: the module state the arm reads) and as the
    product computes it (`arm`: det_i's own tables, the sign at 2288 as in its twins);
  * the time-symmetric finish of off_diagonal_move_chem_cauchySchwarz (4093-4162): `finish`.

tests/golden/README_cauchyschwarz_time_sym.md records where the two arms part and why.  Determinants are (up, dn) pairs of
Python ints; orbitals are 1-based."""
import math

from tests.cauchy_checker import _bits

SQRT2 = math.sqrt(2.0)


class MoveTables:
    """what the move leaves in module state for its parent (2695-2737): cs_sqrt_prime and cs_sqrt_prime_spin per occupied
    orbital (occ_orb order: up ascending then dn ascending, core included) and sum_cs_sqrt_prime over the active electrons"""

    def __init__(self, cs, iu, id_):
        ou, od = _bits(iu), _bits(id_)
        self.prime = [cs._prime(o, ou) for o in ou] + [cs._prime(o, od) for o in od]
        self.spin = [cs._prime_spin(o, ou, od) for o in ou + od]
        s = 0.0
        for v in self.spin[cs.nc:len(ou)]:
            s = s + v
        for v in self.spin[len(ou) + cs.nc:]:
            s = s + v
        self.sum = s


def _diff(a, b):
    """(count, [orbitals of a not in b], [orbitals of b not in a]), ascending; count None if not a 0..2-fold difference"""
    x, y = _bits(a & ~b), _bits(b & ~a)
    if len(x) > 2 or len(x) != len(y):
        return None, x, y
    return len(x), x, y


def _arm(cs, iu, id_, tu, td, tab, sign_2288):
    """is_connected_chem(det_i, target) with proposal_method = 'CauchySchwarz': (connected, level, prob without the level
    factor).  tab: the module's move tables (MoveTables); sign_2288: +1 as the reference has it, -1 as meant"""
    cu, xu, yu = _diff(iu, tu) if iu != tu else (0, [], [])
    if cu is None:
        return False, -1, 0.0
    cd, xd, yd = _diff(id_, td) if id_ != td else (0, [], [])
    if cd is None:
        return False, -1, 0.0
    level = cu + cd
    if level > 2:
        return False, -1, 0.0
    sym, sq, ssum = cs.orbsym, cs.sq, cs.sym
    ne = cs.nelec - 2 * cs.nc
    if level == 1:                                   # 2131-2152
        det, d1, d2 = (iu, xu[0], yu[0]) if cu == 1 else (id_, xd[0], yd[0])
        if sym[d1] != sym[d2]:
            return False, level, 0.0
        i_open = sum(1 for i in range(1, cs.norb + 1) if not (det >> (i - 1)) & 1 and sym[i] == sym[d1])
        return True, 1, 1.0 / ((ne) * (i_open))
    if level != 2:
        return True, level, 0.0
    if cu == 2:
        d1, d2, d3, d4 = xu[0], xu[1], yu[0], yu[1]
    elif cd == 2:
        d1, d2, d3, d4 = xd[0], xd[1], yd[0], yd[1]
    else:
        d1, d2, d3, d4 = xu[0], xd[0], yu[0], yd[0]
    if cs.prod[sym[d1]][sym[d2]] != cs.prod[sym[d3]][sym[d4]]:
        return False, 2, 0.0
    ou, od = _bits(iu), _bits(id_)
    nup = len(ou)
    occ_by = lambda lst, s: [x for x in lst if sym[x] == s]
    n_by = lambda s: len(cs.which[s])
    if cu == 2 or cd == 2:
        up = cu == 2
        own = ou if up else od
        off = 0 if up else nup
        e1, e2 = own.index(d1) + off, own.index(d2) + off          # excite_from_1_i, excite_from_2_i (0-based)
        o1, o2, k, l = d1, d2, d3, d4
        s1 = sym[l]
        i_open = n_by(s1) - len(occ_by(own, s1)) - (1 if s1 == sym[k] else 0)
        if i_open == 0:
            return True, 2, 0.0
        c1, c2, s = tab.spin[e1], tab.spin[e2], tab.sum
        pp = (c1 / s * c2 / (s - c1) + c2 / s * c1 / (s - c2))
        den = 0.0
        for x in occ_by(own, s1):
            den = den + sq[o2][x] + sq[o1][x]
        den = ssum[s1][o2] + ssum[s1][o1] - den
        if s1 == sym[k]:
            den = den - sq[o2][k] - sq[o1][k]
        tmp = (sq[o1][k] + sq[o2][k]) / (tab.prime[e1] + tab.prime[e2]) * (sq[o2][l] + sq[o1][l]) / den
        s1 = sym[k]
        i_open = n_by(s1) - len(occ_by(own, s1)) - (1 if s1 == sym[l] else 0)
        if i_open != 0:
            if s1 == sym[l]:
                den = den + sq[o2][k] - sq[o2][l] + sq[o1][k] - sq[o1][l]
            else:
                den = 0.0
                for x in occ_by(own, s1):
                    if up and sign_2288 > 0:
                        den = den + sq[o2][x] - sq[o1][x]           # 2287-2288 as written
                    else:
                        den = den + sq[o2][x] + sq[o1][x]
                den = ssum[s1][o2] + ssum[s1][o1] - den
            tmp = tmp + (sq[o1][l] + sq[o2][l]) / (tab.prime[e1] + tab.prime[e2]) * (sq[o2][k] + sq[o1][k]) / den
        return True, 2, pp * tmp
    # one up and one dn electron (2383-2444)
    o1, o2, k, l = d1, d2, d3, d4
    e1, e2 = ou.index(o1), od.index(o2) + nup
    s1 = sym[l]
    i_open = n_by(s1) - len(occ_by(od, s1))
    if i_open == 0:
        return True, 2, 0.0
    c1, c2, s = tab.spin[e1], tab.spin[e2], tab.sum
    pp = (c1 / s * c2 / (s - c1) + c2 / s * c1 / (s - c2))
    den = 0.0
    for x in occ_by(od, s1):
        den = den + sq[o2][x] + sq[o1][x]
    den = ssum[s1][o2] + ssum[s1][o1] - den
    tmp = (sq[o1][k] + sq[o2][k]) / (tab.spin[e1] + tab.spin[e2]) * (sq[o2][l] + sq[o1][l]) / den
    den = 0.0
    s1 = sym[k]
    i_open = n_by(s1) - len(occ_by(ou, s1))
    if i_open != 0:
        for x in occ_by(ou, s1):
            den = den + sq[o2][x] + sq[o1][x]
        den = ssum[s1][o2] + ssum[s1][o1] - den
        tmp = tmp + (sq[o1][l] + sq[o2][l]) / (tab.spin[e1] + tab.spin[e2]) * (sq[o2][k] + sq[o1][k]) / den
    return True, 2, pp * tmp


def literal_arm(cs, iu, id_, tu, td, tab=None):
    """the arm as written: the sign at 2288 as it stands and the module tables `tab` (det_i's own when None -- what they hold
    right after a double-excitation proposal from det_i)"""
    return _arm(cs, iu, id_, tu, td, tab if tab is not None else MoveTables(cs, iu, id_), +1)


def arm(cs, iu, id_, tu, td):
    """the arm the product computes (cs_is_connected_prob): det_i's own tables, `+` at 2288"""
    return _arm(cs, iu, id_, tu, td, MoveTables(cs, iu, id_), -1)


def finish(cs, z, tau, iu, id_, ju, jd, level, prob, ham):
    """the time-symmetric end of the move (4093-4162) for a proposal det_i -> det_j of `level` with probability `prob`:
    returns (det_j_up, det_j_dn, weight_j).  ham(iu, id, ju, jd, level): hamiltonian_chem, the plain matrix element."""
    norm_i = SQRT2 if iu == id_ else 1.0
    if (ju == iu and jd == id_) or (jd == iu and ju == id_):
        return ju, jd, 0.0
    p_single = cs.n_single / float(cs.n_total)
    p_double = cs.n_double / float(cs.n_total)
    if ju == jd:
        if z != 1:
            return ju, jd, 0.0
        _, lsym, psym = arm(cs, iu, id_, jd, ju)
        norm_j = 1 / prob
        if lsym == 1:
            prob = (prob + psym * p_single) / 2
        else:
            prob = (prob + psym * p_double) / 2
        norm_j = 2 * norm_j / SQRT2 * (prob)
        me = ham(iu, id_, ju, jd, level)
        me = (norm_j / norm_i) * me
    else:
        norm_j = 1.0
        m1 = ham(iu, id_, ju, jd, level)
        conn, lsym, psym = arm(cs, iu, id_, jd, ju)
        if conn:
            m2 = ham(iu, id_, jd, ju, lsym)
            if lsym == 1:
                prob = prob + (psym * p_single)
            if lsym == 2:
                prob = prob + (psym * p_double)
            me = (norm_j / norm_i) * (m1 + z * m2)
        else:
            me = (norm_j / norm_i) * (m1)
    if ju > jd:
        ju, jd = jd, ju
        me = me * z
    return ju, jd, -tau * me / prob


def move(cs, z, tau, iu, id_, rng, ham):
    """one time-symmetric proposal: (level, det_j_up, det_j_dn, weight_j); level 0 = no move (weight 0, det_j = det_i)"""
    level, ju, jd, p = cs.move(iu, id_, rng)
    if level == 0:
        return 0, ju, jd, 0.0
    ju, jd, w = finish(cs, z, tau, iu, id_, ju, jd, level, p, ham)
    return level, ju, jd, w


def flip_mass(paths):
    """the move's path mass per det_j: {det_j: summed mass}"""
    mass = {}
    for p in paths:
        mass[p[5]] = mass.get(p[5], 0.0) + p[6]
    return mass
