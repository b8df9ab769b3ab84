"""An independent, plain reference for the Hubbard model in its plane-wave basis ('hubbardk'), on top of tests/proposal_checker.py
(second quantisation on bit strings) and of nothing from oracle/ or the HIP library.

Orbital P of spin s is the plane wave of lattice momentum k_P = (kx, ky) in units of pi / L (every component even, defined modulo
(2 l_x, 2 l_y)); H = sum_P eps_P n_P + (U / N) sum a+_{p up} a_{q up} a+_{r dn} a_{s dn} over k_p - k_q + k_r - k_s = 0 modulo the
reciprocal lattice, which in the form of proposal_checker.Hamiltonian (1/2 sum_PQRS v(P,Q,R,S) a+_P a+_R a_S a_Q) is

  t(P, Q) = eps_P delta_PQ,   v(P, Q, R, S) = U / N when P, Q share one spin, R, S share the other and k_P - k_Q + k_R - k_S = 0.

The orbital order is data (the k table): orbital l_y (i-1) + j has k = (-l_x + 2 i, -l_y + 2 j), minus 1 in a direction of odd length,
eps = -2 t (cos(pi kx / l_x) + cos(pi ky / l_y)) (a chain: the long direction's cosine only), ordered by repeatedly taking the first
index that holds the minimum.  The model's spectrum is that of the real-space model, which the tests compare it with."""
import itertools
import math

import numpy as np

from tests import proposal_checker as PC


def k_table(l_x, l_y, t):
    """([(kx, ky)] in units of pi / L, [eps]) in the model's orbital order"""
    ks = []
    for i in range(1, l_x + 1):
        for j in range(1, l_y + 1):
            ks.append((-l_x + 2 * i - (1 if l_x % 2 else 0), -l_y + 2 * j - (1 if l_y % 2 else 0)))
    assert not (l_x == 1 and l_y == 1)

    def eps(k):
        cx, cy = math.cos(math.pi * k[0] / float(l_x)), math.cos(math.pi * k[1] / float(l_y))
        return -2.0 * t * (cx if l_y == 1 else cy if l_x == 1 else cx + cy)
    e = [eps(k) for k in ks]
    left, order = list(range(len(ks))), []
    while left:                              # the first index equal to the minimum, again and again
        m = min(e[i] for i in left)
        first = next(i for i in left if e[i] == m)
        order.append(first); left.remove(first)
    return [ks[i] for i in order], [e[i] for i in order]


class HubbardKH(PC.Hamiltonian):
    def __init__(self, l_x, l_y, t, U, table=None):
        self.l_x, self.l_y, self.norb, self.U = l_x, l_y, l_x * l_y, float(U)
        self.k, self.eps = table if table is not None else k_table(l_x, l_y, float(t))
        self.ubyn = self.U / self.norb
        self.index = {self.fold(k): i for i, k in enumerate(self.k)}
        assert len(self.index) == self.norb

    def fold(self, k):
        return (k[0] % (2 * self.l_x), k[1] % (2 * self.l_y))

    def t(self, P, Q):
        return self.eps[P % self.norb] if P == Q else 0.0

    def v(self, P, Q, R, S):
        n = self.norb
        if P // n != Q // n or R // n != S // n or P // n == R // n:
            return 0.0
        a, b, c, d = self.k[P % n], self.k[Q % n], self.k[R % n], self.k[S % n]
        if self.fold((a[0] - b[0] + c[0] - d[0], a[1] - b[1] + c[1] - d[1])) != (0, 0):
            return 0.0
        return self.ubyn

    def momentum(self, up, dn):
        kx = sum(self.k[o][0] for o in PC._bits(up)) + sum(self.k[o][0] for o in PC._bits(dn))
        ky = sum(self.k[o][1] for o in PC._bits(up)) + sum(self.k[o][1] for o in PC._bits(dn))
        return self.fold((kx, ky))


def triples_hubbardk(H, up, dn):
    """the move's triples, in its order (up electrons x dn electrons x empty up orbitals, all ascending):
    [(p, q, r, s, child)] with s the orbital momentum conservation fixes and child None when s is occupied (a blocked triple)"""
    out = []
    empty = [o for o in range(H.norb) if not up >> o & 1]
    for p in PC._bits(up):
        for q in PC._bits(dn):
            for r in empty:
                kq, kr, kp = H.k[q], H.k[r], H.k[p]
                s = H.index[H.fold((kq[0] - (kr[0] - kp[0]), kq[1] - (kr[1] - kp[1])))]
                child = None if dn >> s & 1 else (up ^ (1 << p) ^ (1 << r), dn ^ (1 << q) ^ (1 << s))
                out.append((p, q, r, s, child))
    return out


def excitations_hubbardk(H, up, dn):
    """every determinant one up and one dn electron away at conserved total momentum"""
    return sorted({c[4] for c in triples_hubbardk(H, up, dn) if c[4] is not None})


def sector(H, nup, ndn, momentum):
    """all determinants of (nup, ndn) electrons with that total momentum (folded), sorted by (up, dn)"""
    strings = lambda n: [sum(1 << o for o in c) for c in itertools.combinations(range(H.norb), n)]
    return sorted((u, d) for u in strings(nup) for d in strings(ndn) if H.momentum(u, d) == H.fold(momentum))


def all_determinants(norb, nup, ndn):
    strings = lambda n: [sum(1 << o for o in c) for c in itertools.combinations(range(norb), n)]
    return sorted((u, d) for u in strings(nup) for d in strings(ndn))


class RingHubbardH(PC.HubbardH):
    """the real-space model on a periodic chain of n >= 3 sites (square_lattice_bonds refuses a direction of length 1)"""

    def __init__(self, n, t, U):
        assert n >= 3
        self.norb, self.t_hop, self.U = n, float(t), float(U)
        self.bonds = sorted(tuple(sorted((s, (s + 1) % n))) for s in range(n))
        self.bonded = set(self.bonds) | {(b, a) for a, b in self.bonds}
        self.nbrs = {s: sorted(b for a, b in self.bonded if a == s) for s in range(n)}


def real_space(l_x, l_y, t, U):
    if l_x == 1 or l_y == 1:
        return RingHubbardH(max(l_x, l_y), t, U)
    return PC.HubbardH(l_x, l_y, True, t, U)


def dense(H, dets, children):
    """the matrix of H among dets: the diagonal and, per determinant, the elements to children(up, dn) that lie in dets.
    (That the children are all there is to a row is what the row test checks, against the element of every pair.)"""
    idx = {d: i for i, d in enumerate(dets)}
    A = np.zeros((len(dets), len(dets)))
    for i, (u, d) in enumerate(dets):
        A[i, i] = H.element(u, d, u, d)[0]
        for c in children(u, d):
            j = idx.get(c)
            if j is not None and j != i:
                A[j, i] = H.element(u, d, c[0], c[1])[0]
    return A


def connections(H, refs, coeffs, eps, diag_mode):
    """what the generator must return, by brute force: per reference determinant with c != 0 its own slot (H_ii c in diag_mode 1,
    else 0; e_mix_den = c) and every child with |H c| > eps (strict), summed per determinant.
    Returns {det: (num, den, n_terms, sum|terms|)} (a determinant's own slot counts the terms of its H_ii); diag_mode 2 (raw) returns the list [(det, num, source index)] in generation order."""
    raw, acc = [], {}
    for i, ((u, d), c) in enumerate(zip(refs, coeffs)):
        if c == 0.0:
            continue
        hd, hn, hs = H.element(u, d, u, d) if diag_mode == 1 else (0.0, 1, 0.0)      # H_ii is itself a sum of hn terms
        raw.append(((u, d), hd * c, float(i)))
        ent = [((u, d), hd * c, c, hn, hs * abs(c))]
        for tr in triples_hubbardk(H, u, d):
            if tr[4] is None:
                continue
            h = H.element(u, d, tr[4][0], tr[4][1])[0]
            if abs(h * c) > eps:
                raw.append((tr[4], h * c, float(i)))
                ent.append((tr[4], h * c, 0.0, 1, abs(h * c)))
        for det, num, den, n, sa in ent:
            a = acc.setdefault(det, [0.0, 0.0, 0, 0.0])
            a[0] += num; a[1] += den; a[2] += n; a[3] += sa
    return raw if diag_mode == 2 else {k: tuple(v) for k, v in acc.items()}
