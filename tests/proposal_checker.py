"""An independent, plain reference for the off-diagonal proposals: Hamiltonian matrix elements from second quantisation, the
exact row of a parent determinant, and the statistics that compare a sample of proposals with that row.

Nothing here comes from oracle/ or from the HIP library, and nothing uses the Slater-Condon rules (they are what is under
test).  A determinant is the pair of bit strings (up, dn); spin orbital P = p for an up electron in orbital p (bit p of up),
norb + p for a down electron: all up orbitals in front of all down orbitals, the order in which the project multiplies the
two strings' permutation factors.  An operator acts on the 2 norb-bit string and picks up (-1)^(occupied spin orbitals below
it), counted on the bits.  H = sum_PQ t(P,Q) a+_P a_Q + 1/2 sum_PQRS v(P,Q,R,S) a+_P a+_R a_S a_Q + constant, with

  chemistry  t = h_pq, v = (pq|rs) (chemists' notation, 8-fold symmetric), both diagonal in spin, constant = the core energy;
             integrals read from the FCIDUMP, records with |value| <= 1e-9 left out as the project's readers leave them out;
  HEG        plane waves k = 2 pi n / L, t = k^2 / 2, v = 1 / (pi L |n_p - n_q|^2) when n_p - n_q = n_s - n_r != 0 (the q = 0
             term is dropped with the background); the Madelung constant is NOT part of H: the project reports it on its own
             line ('HF energy including Madelung', tests/test_formats.py) and the walk's H is without it;
  Hubbard    t = -t_hop on every lattice bond (both directions), v = U for the four indices on one site.

Orbital order, k-point order and site numbering enter as data (a permutation / a table), not as code.
With time-reversal symmetry a state is a representative (up <= dn): |u,u> or (|u,d> + z |d,u>) / sqrt(2)."""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------- operators on bit strings


def _pop(x):
    return bin(x).count("1")


def _bits(x):
    out, k = [], 0
    while x:
        if x & 1:
            out.append(k)
        x >>= 1; k += 1
    return out


def _ann(state, P):
    """a_P |state>: (state, sign) or None"""
    b = 1 << P
    if not state & b:
        return None
    return state ^ b, -1 if _pop(state & (b - 1)) & 1 else 1


def _cre(state, P):
    b = 1 << P
    if state & b:
        return None
    return state | b, -1 if _pop(state & (b - 1)) & 1 else 1


class Hamiltonian:
    """<J| H |I> by applying every operator string of H to |I> that can end in |J>.  Subclasses give t, v and the constant."""
    norb = 0
    const = 0.0

    def t(self, P, Q):
        raise NotImplementedError

    def v(self, P, Q, R, S):
        raise NotImplementedError

    def state(self, up, dn):
        return int(up) | (int(dn) << self.norb)

    def terms(self, iu, id_, ju, jd):
        """every non-zero term of <ju,jd| H |iu,id>"""
        I, J = self.state(iu, id_), self.state(ju, jd)
        out = []
        if I == J and self.const != 0.0:
            out.append(self.const)
        if _pop(I) != _pop(J) or _pop(I & ~J) > 2:
            return out                      # no string of at most two annihilators and two creators joins them
        occ = _bits(I)
        for Q in occ:                       # a+_P a_Q
            K, s1 = _ann(I, Q)
            if K & ~J:
                continue
            rest = J & ~K
            if _pop(rest) != 1:
                continue
            P = _bits(rest)[0]
            _, s2 = _cre(K, P)
            val = self.t(P, Q)
            if val != 0.0:
                out.append(s1 * s2 * val)
        for Q in occ:                       # 1/2 a+_P a+_R a_S a_Q: a_Q first
            K1, s1 = _ann(I, Q)
            for S in _bits(K1):
                K2, s2 = _ann(K1, S)
                if K2 & ~J:
                    continue
                rest = _bits(J & ~K2)
                if len(rest) != 2:
                    continue
                for R, P in ((rest[0], rest[1]), (rest[1], rest[0])):
                    K3, s3 = _cre(K2, R)
                    _, s4 = _cre(K3, P)
                    val = self.v(P, Q, R, S)
                    if val != 0.0:
                        out.append(0.5 * (s1 * s2 * s3 * s4) * val)
        return out

    def element(self, iu, id_, ju, jd):
        """(<J|H|I>, number of terms, sum of |terms|)"""
        tm = self.terms(iu, id_, ju, jd)
        return math.fsum(tm), len(tm), math.fsum(abs(x) for x in tm)

    # -- time-reversal representatives
    def _components(self, up, dn, z):
        """(weight exponent, up, dn, sign): the state is sum sign * 2^(-exponent/2) |up, dn>"""
        if up == dn:
            return [(0, up, dn, 1)]
        return [(1, up, dn, 1), (1, dn, up, z)]

    def element_ts(self, iu, id_, ju, jd, z=1):
        """the element between two representatives, from the up-to-four raw elements and the explicit normalisation: an
        open-shell side contributes 1/sqrt(2), so the product of the two is 1, 1/sqrt(2) or 1/2"""
        tm = []
        for ea, au, ad, sa in self._components(iu, id_, z):
            for eb, bu, bd, sb in self._components(ju, jd, z):
                c = (1.0, math.sqrt(0.5), 0.5)[ea + eb] * sa * sb
                tm.extend(c * x for x in self.terms(au, ad, bu, bd))
        return math.fsum(tm), len(tm), math.fsum(abs(x) for x in tm)


def rounding_bound(n_terms, sum_abs):
    """the derived bound on |H_kernel - H_reference|: a double-precision sum of n terms in any order, each term itself a
    product or two, stays within 4 n 2^-53 sum|terms| of the exact sum"""
    return 4.0 * n_terms * 2.0 ** -53 * sum_abs


# ---------------------------------------------------------------------------------------------- the three Hamiltonians
def read_fcidump(path, drop_below=1e-9):
    """(norb, {(p,q): h_pq}, {canonical (pq|rs) key: value}, core energy), orbitals 1-based as in the file"""
    one, two, core, norb = {}, {}, 0.0, None
    with open(path) as f:
        header = True
        for line in f:
            if header:
                u = line.upper()
                if "NORB" in u:
                    norb = int(u.split("NORB")[1].lstrip(" =").split(",")[0])
                if "&END" in u or "/" in line:
                    header = False
                continue
            t = line.split()
            if len(t) != 5:
                continue
            val, (p, q, r, s) = float(t[0]), (int(x) for x in t[1:])
            if not abs(val) > drop_below:
                continue
            if p == q == r == s == 0:
                core = val
            elif r == 0 and s == 0:
                one[(max(p, q), min(p, q))] = val
            else:
                two[_eri_key(p, q, r, s)] = val
    return norb, one, two, core


def _eri_key(p, q, r, s):
    a, b = (p, q) if p >= q else (q, p)
    c, d = (r, s) if r >= s else (s, r)
    return (a, b, c, d) if (a, b) >= (c, d) else (c, d, a, b)


class ChemH(Hamiltonian):
    """orb_order[i] = the file's (1-based) orbital that bit i of a determinant stands for"""

    def __init__(self, fcidump, orb_order):
        self.norb, self.h1, self.h2, self.const = read_fcidump(fcidump)
        self.file_orb = [int(x) for x in orb_order]
        assert sorted(self.file_orb) == list(range(1, self.norb + 1))

    def t(self, P, Q):
        n = self.norb
        if P // n != Q // n:
            return 0.0
        p, q = self.file_orb[P % n], self.file_orb[Q % n]
        return self.h1.get((max(p, q), min(p, q)), 0.0)

    def v(self, P, Q, R, S):
        n = self.norb
        if P // n != Q // n or R // n != S // n:
            return 0.0
        f = self.file_orb
        return self.h2.get(_eri_key(f[P % n], f[Q % n], f[R % n], f[S % n]), 0.0)


class HegH(Hamiltonian):
    """k_vectors[norb, 3] in the system's orbital order (data), cell length L; three dimensions"""

    def __init__(self, k_vectors, length_cell):
        kv = np.asarray(k_vectors, float)
        self.norb, self.L = len(kv), float(length_cell)
        unit = 2.0 * math.pi / self.L
        self.n = [tuple(int(round(x / unit)) for x in row[:3]) for row in kv]
        assert all(abs(x / unit - round(x / unit)) < 1e-9 for row in kv for x in row[:3])
        assert len(set(self.n)) == self.norb
        self.unit = unit
        self.index = {n: i for i, n in enumerate(self.n)}

    def t(self, P, Q):
        if P != Q:
            return 0.0
        n = self.n[P % self.norb]
        return 0.5 * self.unit * self.unit * (n[0] * n[0] + n[1] * n[1] + n[2] * n[2])

    def v(self, P, Q, R, S):
        m = self.norb
        if P // m != Q // m or R // m != S // m:
            return 0.0
        a, b, c, d = self.n[P % m], self.n[Q % m], self.n[R % m], self.n[S % m]
        q = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
        if q != (d[0] - c[0], d[1] - c[1], d[2] - c[2]):
            return 0.0
        q2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
        if q2 == 0:
            return 0.0
        return 1.0 / (math.pi * self.L * q2)


def square_lattice_bonds(l_x, l_y, pbc):
    """bonds of the l_x by l_y lattice, site (x, y) -> y l_x + x (0-based), each bond once (lengths above 2 when periodic)"""
    assert not pbc or (l_x > 2 and l_y > 2)
    bonds = set()
    for y in range(l_y):
        for x in range(l_x):
            s = y * l_x + x
            if x + 1 < l_x or pbc:
                bonds.add(tuple(sorted((s, y * l_x + (x + 1) % l_x))))
            if y + 1 < l_y or pbc:
                bonds.add(tuple(sorted((s, ((y + 1) % l_y) * l_x + x))))
    return sorted(bonds)


class HubbardH(Hamiltonian):
    def __init__(self, l_x, l_y, pbc, t, U):
        self.norb, self.t_hop, self.U = l_x * l_y, float(t), float(U)
        self.bonds = square_lattice_bonds(l_x, l_y, pbc)
        self.bonded = set(self.bonds) | {(b, a) for a, b in self.bonds}
        self.nbrs = {s: sorted(b for a, b in self.bonded if a == s) for s in range(self.norb)}

    def t(self, P, Q):
        n = self.norb
        if P // n != Q // n or (P % n, Q % n) not in self.bonded:
            return 0.0
        return -self.t_hop

    def v(self, P, Q, R, S):
        n = self.norb
        if P // n != Q // n or R // n != S // n:
            return 0.0
        return self.U if P % n == Q % n == R % n == S % n else 0.0


# ---------------------------------------------------------------------------------------------- the exact row of a parent
def _singles(det, norb, frozen=0):
    occ = [o for o in _bits(det) if o >= frozen]
    emp = [o for o in range(norb) if not (det >> o) & 1]
    return [det ^ (1 << a) ^ (1 << b) for a in occ for b in emp]


def _doubles(det, norb, frozen=0):
    occ = [o for o in _bits(det) if o >= frozen]
    emp = [o for o in range(norb) if not (det >> o) & 1]
    return [det ^ (1 << a) ^ (1 << b) ^ (1 << c) ^ (1 << d) for i, a in enumerate(occ) for b in occ[i + 1:]
            for k, c in enumerate(emp) for d in emp[k + 1:]]


def excitations_chem(up, dn, norb, n_core_orb=0):
    """every single and double excitation of (up, dn); the lowest n_core_orb orbitals of each spin stay occupied"""
    su, sd = _singles(up, norb, n_core_orb), _singles(dn, norb, n_core_orb)
    out = [(a, dn) for a in su] + [(up, b) for b in sd]
    out += [(a, dn) for a in _doubles(up, norb, n_core_orb)] + [(up, b) for b in _doubles(dn, norb, n_core_orb)]
    out += [(a, b) for a in su for b in sd]
    return out


def excitations_heg(H, up, dn):
    """every double excitation that conserves momentum (H holds no other off-diagonal term)"""
    m = H.norb
    I = H.state(up, dn)
    occ = _bits(I)
    out = set()
    for i, Q in enumerate(occ):
        for S in occ[i + 1:]:
            nq, ns = H.n[Q % m], H.n[S % m]
            tot = (nq[0] + ns[0], nq[1] + ns[1], nq[2] + ns[2])
            K = I ^ (1 << Q) ^ (1 << S)
            for p in range(m):
                P = p + m * (Q // m)
                if K >> P & 1:
                    continue
                np_ = H.n[p]
                r = H.index.get((tot[0] - np_[0], tot[1] - np_[1], tot[2] - np_[2]))
                if r is None:
                    continue
                R = r + m * (S // m)
                if R == P or K >> R & 1:
                    continue
                J = K | (1 << P) | (1 << R)
                if J != I:
                    out.add((J & ((1 << m) - 1), J >> m))
    return sorted(out)


def excitations_hubbard(H, up, dn):
    out = set()
    for s in range(H.norb):
        for nb in H.nbrs[s]:
            if up >> s & 1 and not up >> nb & 1:
                out.add((up ^ (1 << s) ^ (1 << nb), dn))
            if dn >> s & 1 and not dn >> nb & 1:
                out.add((up, dn ^ (1 << s) ^ (1 << nb)))
    return sorted(out)


def representative(up, dn):
    return (up, dn) if up <= dn else (dn, up)


def row(H, parent, children, time_sym=False, z=1):
    """{child: (H_ij, n_terms, sum|terms|)} over the children (mapped to representatives and merged when time_sym), the
    parent itself left out, zero elements kept"""
    iu, id_ = parent
    out = {}
    for c in children:
        if time_sym:
            c = representative(*c)
            if z != 1 and c[0] == c[1]:
                continue
        if c == (iu, id_) or c in out:
            continue
        out[c] = H.element_ts(iu, id_, c[0], c[1], z) if time_sym else H.element(iu, id_, c[0], c[1])
    return out


# ---------------------------------------------------------------------------------------------- statistics
POOL_BELOW = 5.0           # cells with a smaller expectation are pooled (tests/test_gpu_cauchy_schwarz.py)
P_MIN = 1e-6               # the G-test passes when chi2.sf(G, dof) > P_MIN at the fixed seeds
N_SIGMA = 5.0
MIN_VISITS = 50            # a child's first moment is tested from this many visits on
MAX_POOLED_MASS = 0.01


def splitmix_states(n):
    """48-bit rannyu states, one per proposal: splitmix64 of the proposal index (the recipe of the Cauchy-Schwarz test)"""
    st = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    st ^= st >> np.uint64(30); st *= np.uint64(0xBF58476D1CE4E5B9)
    st ^= st >> np.uint64(27); st *= np.uint64(0x94D049BB133111EB); st ^= st >> np.uint64(31)
    return st & np.uint64((1 << 48) - 1)


def state_limbs(st):
    st = np.asarray(st, np.uint64)
    return np.stack([(st >> np.uint64(36)) & np.uint64(4095), (st >> np.uint64(24)) & np.uint64(4095),
                     (st >> np.uint64(12)) & np.uint64(4095), st & np.uint64(4095)], axis=1).astype(np.int32)


def g_test(obs, expv):
    """(G, degrees of freedom, p, share of the expectation that was pooled): cells below POOL_BELOW pooled into one"""
    from scipy.stats import chi2
    obs, expv = np.asarray(obs, float), np.asarray(expv, float)
    small = expv < POOL_BELOW
    o = np.append(obs[~small], obs[small].sum()); e = np.append(expv[~small], expv[small].sum())
    keep = e > 0
    o, e = o[keep], e[keep]
    G = 2.0 * np.sum(np.where(o > 0, o * np.log(np.where(o > 0, o, 1) / e), 0.0))
    dof = len(o) - 1
    return float(G), dof, float(chi2.sf(G, dof)), float(expv[small].sum() / max(expv.sum(), 1.0))


def tally(ju, jd, w):
    """per distinct (ju, jd) among the entries with w != 0: keys, visits, sum w, sum w^2, min w, max w"""
    ju, jd, w = np.asarray(ju, np.uint64).ravel(), np.asarray(jd, np.uint64).ravel(), np.asarray(w, float).ravel()
    nz = w != 0.0
    ju, jd, w = ju[nz], jd[nz], w[nz]
    order = np.lexsort((jd, ju))
    ju, jd, w = ju[order], jd[order], w[order]
    if len(w) == 0:
        return [], np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)
    first = np.concatenate(([True], (ju[1:] != ju[:-1]) | (jd[1:] != jd[:-1])))
    start = np.nonzero(first)[0]
    keys = list(zip(ju[start].tolist(), jd[start].tolist()))
    cnt = np.diff(np.append(start, len(w))).astype(float)
    return keys, cnt, np.add.reduceat(w, start), np.add.reduceat(w * w, start), np.minimum.reduceat(w, start), np.maximum.reduceat(w, start)


def is_live(v):
    """v = (H_ij, n_terms, sum|terms|).  An element inside its own rounding bound is a zero that the summation order did not cancel
    exactly (1e-17 where the terms are 1e-2): the kernel's value there is rounding noise of another order, and so is the weight it
    returns.  Only elements above the bound count as connections."""
    return abs(v[0]) > rounding_bound(v[1], v[2])


class _Sample:
    """the tally of a sample, per distinct weighted child, next to the row's elements for those children"""

    def __init__(self, rowd, ju, jd, w):
        self.ju, self.jd, self.w = np.asarray(ju, np.uint64), np.asarray(jd, np.uint64), np.asarray(w, float)
        self.N = self.w.shape[0]
        self.keys, self.cnt, self.S, self.S2, self.wmin, self.wmax = tally(self.ju, self.jd, self.w)
        self.outside = [k for k in self.keys if k not in rowd]
        known = [rowd.get(k, (0.0, 0, 0.0)) for k in self.keys]
        self.hij = np.array([v[0] for v in known])
        self.live = np.array([is_live(v) for v in known], bool)
        self.visited = set(self.keys)


def _check_closure(rowd, sm, parent, nelec, time_sym):
    """1. every weighted child is in the row, on a live element (rounding noise on a zero-within-rounding aside); a whole
    determinant returned without weight is in the row too, and not on a live element"""
    fails = []
    if sm.outside:
        fails.append(("closure", "%d weighted children outside the row, e.g. %s" % (len(sm.outside), sm.outside[:3])))
    dead = [k for k, sk, l in zip(sm.keys, sm.S, sm.live) if k in rowd and not l and abs(sk) / sm.N > 1e-12]
    if dead:
        fails.append(("closure", "%d children carry weight where H_ij = 0, e.g. %s" % (len(dead), dead[:3])))
    if time_sym and any(a > b for a, b in sm.keys):
        fails.append(("closure", "a weighted child is not a representative"))
    zero = sm.w.ravel() == 0.0
    lost = set()
    if np.any(zero):
        for a, b in np.unique(np.stack([sm.ju.ravel()[zero], sm.jd.ravel()[zero]], axis=1), axis=0).tolist():
            if (_pop(a), _pop(b)) != tuple(nelec):
                continue                    # a partly built determinant: no move
            c = representative(a, b) if time_sym else (a, b)
            if c == tuple(parent):
                continue
            if c not in rowd:
                fails.append(("closure", "a weightless child outside the row: %s" % (c,)))
            elif is_live(rowd[c]):
                lost.add(c)
    if lost:
        fails.append(("closure", "%d connected children were returned with weight 0, e.g. %s" % (len(lost), sorted(lost)[:3])))
    return fails


def _check_weights_and_distribution(sm, tau, rep):
    """2. one weight per live child, of sign -sign(H_ij), implied probability -tau H_ij / w in (0, 1], summing to at most 1;
    3. the visits against N p_j, everything else (weightless proposals, visits to zeros-within-rounding) one more cell"""
    fails, N, l = [], sm.N, sm.live
    keys = [k for k, x in zip(sm.keys, l) if x]
    cnt, hij, wmin, wmax = sm.cnt[l], sm.hij[l], sm.wmin[l], sm.wmax[l]
    if np.any(wmin != wmax):
        k = int(np.argmax(wmax - wmin))
        fails.append(("weight", "the weight on %s varies between visits: %r .. %r" % (keys[k], wmin[k], wmax[k])))
    if np.any(np.sign(wmin) != -np.sign(hij)):
        fails.append(("weight", "a weight's sign is not -sign(H_ij)"))
    p = -tau * hij / wmin
    rep["sum_p"] = float(p.sum())
    if not (np.all(p > 0) and np.all(p <= 1.0) and p.sum() <= 1.0 + 1e-12):
        fails.append(("weight", "implied probabilities outside (0, 1] or summing to %r" % float(p.sum())))
    n_null = N - int(cnt.sum())
    rep["null_seen"], rep["null_expected"] = n_null / N, 1.0 - float(p.sum())
    G, dof, pv, pooled = g_test(np.append(cnt, n_null), np.append(p, max(1.0 - p.sum(), 0.0)) * N)
    rep.update(G=G, dof=dof, p=pv, pooled=pooled)
    if not pv > P_MIN:
        worst = np.argsort(-np.abs(cnt - N * p) / np.sqrt(np.maximum(N * p, 1.0)))[:5]
        fails.append(("distribution", "G = %.1f on %d dof, p = %.3g; worst cells %s; null %d against %.1f" % (
            G, dof, pv, [(keys[k], cnt[k], N * p[k]) for k in worst], n_null, N * (1 - p.sum()))))
    if not pooled < MAX_POOLED_MASS:
        fails.append(("pooled", "%.3g of the probability mass sits in the pooled cell" % pooled))
    return fails


def _check_reach(rowd, sm, table_prob, rep):
    """4. every live element was visited.  With table_prob (a move that may leave connected determinants aside) an unvisited one
    must be one the move's own tables give no or hardly any probability: a determinant of probability p stays unvisited with
    probability exp(-N p), which is beyond 5 sigma (5.7e-7) when N p > 14.4"""
    fails = []
    unreached = [k for k, v in rowd.items() if is_live(v) and k not in sm.visited]
    rep["unreached"] = len(unreached)
    if unreached and table_prob is None:
        fails.append(("reach", "%d connected determinants were never proposed, e.g. %s" % (len(unreached), unreached[:3])))
    if unreached and table_prob is not None:
        probs = {k: table_prob(k) for k in unreached}
        rep["unreached_list"] = [(k, rowd[k][0], probs[k]) for k in unreached]
        rep["unreached_by_table"] = sum(1 for k in unreached if probs[k] == 0.0)
        late = [(k, sm.N * probs[k]) for k in unreached if sm.N * probs[k] > -math.log(5.7e-7)]
        if late:
            fails.append(("reach", "%d determinants were never proposed although the tables expect them often: %s" % (len(late), late[:5])))
    return fails


def _check_moments(rowd, sm, tau, rep):
    """5. the mean weight on every child with MIN_VISITS visits or more within N_SIGMA standard errors (+ 1e-12) of -tau H_ij,
    and the row total within N_SIGMA of its own standard errors; worst_z is reported over the live elements"""
    fails, N = [], sm.N
    mean = sm.S / N
    se = np.sqrt(np.maximum(sm.S2 / N - mean * mean, 0.0) / N)
    tested = sm.cnt >= MIN_VISITS
    dev = np.abs(mean + tau * sm.hij)
    zsc = np.where(tested & sm.live, dev / np.where(se > 0, se, 1.0), 0.0)
    rep["worst_z"] = float(zsc.max()) if len(zsc) else 0.0
    rep["tested"] = int(tested.sum())
    bad = tested & ~(dev <= N_SIGMA * se + 1e-12)
    if np.any(bad):
        k = int(np.argmax(np.where(bad, dev / np.where(se > 0, se, 1.0), 0.0)))
        fails.append(("moment", "%d children off by more than %g se; worst %s: mean %r against %r, se %r" % (
            int(bad.sum()), N_SIGMA, sm.keys[k], mean[k], -tau * sm.hij[k], se[k])))
    tot = sm.w.reshape(N, -1).sum(axis=1)
    want = -tau * math.fsum(v[0] for v in rowd.values())
    tse = float(tot.std(ddof=1) / math.sqrt(N))
    rep["total_z"] = abs(float(tot.mean()) - want) / tse if tse > 0 else 0.0
    if not abs(float(tot.mean()) - want) <= N_SIGMA * tse:
        fails.append(("total", "row total %r against %r, se %r" % (float(tot.mean()), want, tse)))
    return fails


def analyse(rowd, parent, ju, jd, w, tau, nelec, weight_by_child=True, time_sym=False, table_prob=None):
    """The five checks of a sample of N proposals from `parent` against its exact row.

    ju, jd, w: arrays of shape (N,) or (N, slots) (heat-bath returns up to two determinants per proposal); nelec = (nup, ndn).
    weight_by_child: the move's weight is a function of the child alone (uniform chemistry, HEG, Hubbard): checks 2 and 3 run.
    table_prob(child) -> the move's own proposal probability, for the doors that may leave connected determinants unproposed.
    Returns (failures, report): failures is a list of (check, text); report holds G, dof, p, pooled, worst_z, null fractions."""
    sm = _Sample(rowd, ju, jd, w)
    rep = {"N": sm.N, "row": len(rowd), "connected": sum(1 for v in rowd.values() if is_live(v)),
           "nonzero": sum(1 for v in rowd.values() if v[0] != 0.0)}
    fails = _check_closure(rowd, sm, parent, nelec, time_sym)
    if sm.outside:
        return fails, rep                   # the other checks need every child's element
    if weight_by_child:
        fails += _check_weights_and_distribution(sm, tau, rep)
    fails += _check_reach(rowd, sm, table_prob, rep)
    fails += _check_moments(rowd, sm, tau, rep)
    return fails, rep


def summary(tag, rep):
    return "%-28s N=%d row=%d connected=%d G=%s dof=%s p=%s worst_z=%.2f total_z=%.2f unreached=%d pooled=%s null=%s/%s" % (
        tag, rep["N"], rep["row"], rep["connected"], "%.1f" % rep["G"] if "G" in rep else "-", rep.get("dof", "-"),
        "%.3g" % rep["p"] if "p" in rep else "-", rep.get("worst_z", float("nan")), rep.get("total_z", float("nan")), rep.get("unreached", -1),
        "%.2g" % rep["pooled"] if "pooled" in rep else "-", "%.4f" % rep["null_seen"] if "null_seen" in rep else "-",
        "%.4f" % rep["null_expected"] if "null_expected" in rep else "-")


# ---------------------------------------------------------------------------------------------- the fixed parents of the tests
def _largest(rowd, want):
    """the child with the largest |H_ij| among those that `want` accepts (ties: the smallest determinant)"""
    cand = [(-abs(v[0]), k) for k, v in rowd.items() if v[0] != 0.0 and want(k)]
    assert cand
    return min(cand)[1]


def parents_chem(H, hf, norb, time_sym=False, z=1):
    """[(name, parent)]: HF, an open-shell single, a double with up != dn (representatives when time_sym: a closed-shell and
    open-shell ones)"""
    r = row(H, hf, excitations_chem(hf[0], hf[1], norb), time_sym, z)
    level = lambda k: min(_pop(hf[0] & ~k[0]) + _pop(hf[1] & ~k[1]), _pop(hf[0] & ~k[1]) + _pop(hf[1] & ~k[0])) if time_sym else \
        _pop(hf[0] & ~k[0]) + _pop(hf[1] & ~k[1])
    single = _largest(r, lambda k: level(k) == 1 and k[0] != k[1])
    double = _largest(r, lambda k: level(k) == 2 and k[0] != k[1] and k[0] != hf[0] and k[1] != hf[1])
    return [("hf", tuple(hf)), ("open_single", single), ("open_double", double)]


def parents_heg(H, hf):
    r = row(H, hf, excitations_heg(H, *hf))
    return [("hf", tuple(hf)), ("off_fermi_sphere", _largest(r, lambda k: True))]


def parents_hubbard(H, neel):
    """the Neel state, the state three hops on that has the most doubly occupied sites, and two packed rows of each spin that
    overlap on one row (electrons with four, some and no free neighbours)"""
    cur = tuple(neel)
    for _ in range(3):
        cur = min((-_pop(a & b), (a, b)) for a, b in excitations_hubbard(H, *cur))[1]
    return [("neel", tuple(neel)), ("three_hops", cur), ("packed_rows", (0x00FF, 0x0FF0))]


# ---------------------------------------------------------------------------------------------- one real step, in expectation
MIN_REPEATS_SEEN = 8       # a determinant seen in fewer repeats goes into one pooled total


def projector_row(rowd, h_ii, tau, e_trial, reweight_factor_inv):
    """the row of the projector a non-semistochastic step applies to a unit weight on the parent:
    delta_ij (1 + tau (E_T - H_ii)) - tau H_ij (1 - delta_ij), times reweight_factor_inv; key None is the parent"""
    out = {k: -tau * v[0] * reweight_factor_inv for k, v in rowd.items()}
    out[None] = (1.0 + tau * (e_trial - h_ii)) * reweight_factor_inv
    return out


def analyse_step_repeats(expected, parent, repeats, quantum=0.0):
    """repeats: one {(up, dn): weight / W} per repeat of the step.  The mean over repeats of every determinant seen in at least
    MIN_REPEATS_SEEN of them within N_SIGMA standard errors (from the spread over the repeats) of the projector row; all the
    other determinants of the row as one total; nothing outside the row.  quantum: the smallest non-zero |weight| / W the step
    can leave on a determinant (min_wt reweight_factor_inv / W under join_walker2).  The pooled determinants arrive as rare
    events of at least that size, and a spread sampled from a handful of events (or none) is no standard error: the pooled
    total's standard error is not taken below the Poisson one, sqrt(sum|expected| quantum / R).  Returns (failures, report)."""
    R = len(repeats)
    fails = []
    seen = {}
    for r in repeats:
        for k in r:
            seen[k] = seen.get(k, 0) + 1
    parent = tuple(parent)
    outside = [k for k in seen if k != parent and k not in expected]
    if outside:
        fails.append(("closure", "%d determinants outside the row after the step, e.g. %s" % (len(outside), outside[:3])))
    worst, tested = 0.0, 0
    pooled = np.zeros(R)
    pooled_expect = []
    for k, want in expected.items():
        det = parent if k is None else k
        if seen.get(det, 0) < MIN_REPEATS_SEEN:
            pooled += np.array([r.get(det, 0.0) for r in repeats])
            pooled_expect.append(want)
            continue
        x = np.array([r.get(det, 0.0) for r in repeats])
        se = float(x.std(ddof=1) / math.sqrt(R))
        dev = abs(float(x.mean()) - want)
        tested += 1
        if se > 1e-14 * abs(want):             # (the parent's own weight is the same in every repeat)
            worst = max(worst, dev / se)
        if not dev <= N_SIGMA * se + 1e-15 * abs(want):
            fails.append(("moment", "%s: mean %r against %r, se %r over %d repeats" % (det, float(x.mean()), want, se, R)))
    want = math.fsum(pooled_expect)
    spread, floor = float(pooled.std(ddof=1) / math.sqrt(R)), math.sqrt(math.fsum(abs(x) for x in pooled_expect) * quantum / R)
    se = max(spread, floor)
    pz = abs(float(pooled.mean()) - want) / se if se > 0 else 0.0
    if not abs(float(pooled.mean()) - want) <= N_SIGMA * se + 1e-15:
        fails.append(("pooled", "rarely seen determinants: total %r against %r, se %r" % (float(pooled.mean()), want, se)))
    return fails, dict(R=R, tested=tested, worst_z=worst, pooled_z=pz, n_pooled=len(pooled_expect), pooled_spread=spread, pooled_floor=floor,
                       pooled_error="Poisson floor" if floor > spread else "sampled spread")


def step_summary(tag, parent, rep):
    return "%s parent %s: %d determinants tested, worst z = %.2f; %d pooled, z = %.2f against the %s (spread %.3g, floor %.3g)" % (
        tag, tuple(hex(x) for x in parent), rep["tested"], rep["worst_z"], rep["n_pooled"], rep["pooled_z"], rep["pooled_error"],
        rep["pooled_spread"], rep["pooled_floor"])
