"""An independent yardstick for the orbital gradient and the diagonal orbital Hessian of sqmc_gpu_orbital_gradient.  Nothing here comes
from sqmc_amd/ or oracle/, and the derivatives use none of the door's formulas: they are read off the energy itself.

Conventions (0-based orbitals): h[p, r]; eri[p, r, q, s] = (pr|qs) in chemists' notation; D[p, r] the spin-summed one-body matrix;
G[p, q, r, s] the spin-free two-body matrix.  E = sum_pr h[p,r] D[p,r] + 1/2 sum_pqrs (pr|qs) G[p,q,r,s] (+ const n2, which no rotation
moves).  A rotation U defines the new orbitals new_P = sum_k U[k, P] old_k, so
    h'[P,Q] = sum_ab U[a,P] U[b,Q] h[a,b],    (PQ|RS)' = sum_abcd U[a,P] U[b,Q] U[c,R] U[d,S] (ab|cd)
and E(U) is the energy of the FIXED D, G on the rotated integrals.  plane_rotation(n, p, q, theta) = exp(theta (e_p e_q^T - e_q e_p^T)):
U_pp = U_qq = cos, U_pq = sin, U_qp = -sin.

Along a plane rotation every one of the four factors U is linear in (cos theta, sin theta), so E(theta) is a trigonometric polynomial
of degree at most 4: nine samples at theta_j = 2 pi j / 9 determine it, a discrete Fourier sum gives a_k, b_k exactly (to rounding)
and  E'(0) = sum_k k b_k,  E''(0) = -sum_k k^2 a_k  -- no step size, no truncation error.

Two evaluations of E(theta), both in longdouble:
  energy(h, eri, D, G, U)        the integrals transformed by einsum, index by index (O(n^5));
  plane_samples(...)             the same sum with U = 1 + V, V non-zero on the 2 x 2 block {p, q} only: the product of the four
                                 factors (1 + V) is expanded into its 15 patterns with at least one V; a pattern with V on the slots S
                                 needs  M_S = sum over the other slots of  T[a_S, rest] W[P_S, rest]  once (no theta in it), and the
                                 pattern without V is E(0).  Exact algebra, O(n^3) per pair; test_orbopt_checker holds the two together.

fock_literal is the literal formula of the Fock matrix (it is an output defined by formula, not a derivative), and the *_abs functions
are the term-by-term sums of absolute values behind the rounding bounds."""
import math
from itertools import combinations

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
PI = LD(4) * np.arctan(LD(1))          # np.pi is a double: the sample angles must be 2 pi j / 9 to longdouble precision
ANGLES = 9


# ----------------------------------------------------------------------------------------------------------------- integrals from a file
def read_fcidump_dense(path, orb_order=None):
    """(h, eri, core) dense from an FCIDUMP, this module's own reader.  orb_order[k] = the file's 1-based orbital that orbital k stands
    for (None: the file's order)"""
    norb, recs, header = None, [], True
    with open(path) as f:
        for line in f:
            if header:
                u = line.upper()
                if "NORB" in u:
                    norb = int(u.split("NORB")[1].lstrip(" =").split(",")[0])
                if "&END" in u or "/" in line:
                    header = False
                continue
            t = line.split()
            if len(t) == 5:
                recs.append((float(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[4])))
    order = list(range(1, norb + 1)) if orb_order is None else [int(x) for x in orb_order]
    assert sorted(order) == list(range(1, norb + 1))
    pos = {f: k for k, f in enumerate(order)}
    h, eri, core = np.zeros((norb, norb)), np.zeros((norb,) * 4), 0.0
    for v, p, q, r, s in recs:
        if p == q == r == s == 0:
            core = v
        elif r == 0 and s == 0:
            a, b = pos[p], pos[q]
            h[a, b] = h[b, a] = v
        else:
            a, b, c, d = pos[p], pos[q], pos[r], pos[s]
            for w, x, y, z in ((a, b, c, d), (b, a, c, d), (a, b, d, c), (b, a, d, c), (c, d, a, b), (d, c, a, b), (c, d, b, a), (d, c, b, a)):
                eri[w, x, y, z] = v
    return h, eri, core


def random_system(norb, seed, symmetric_g=True):
    """seeded dense h, eri with the 8-fold symmetry of real integrals, a symmetric D, and G symmetrised to G[p,q,r,s] = G[r,s,p,q] =
    G[q,p,s,r] (or left as drawn)"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1.0, 1.0, (norb, norb)); h = h + h.T
    e = rng.uniform(-1.0, 1.0, (norb,) * 4)
    e = e + e.transpose(1, 0, 2, 3); e = e + e.transpose(0, 1, 3, 2); e = e + e.transpose(2, 3, 0, 1)
    D = rng.uniform(-1.0, 1.0, (norb, norb)); D = D + D.T
    G = rng.uniform(-1.0, 1.0, (norb,) * 4)
    if symmetric_g:
        G = G + G.transpose(2, 3, 0, 1); G = G + G.transpose(1, 0, 3, 2)
    return h, e, D, G


# --------------------------------------------------------------------------------------------------------------------------- the energy
def plane_rotation(n, p, q, theta):
    U = np.eye(n, dtype=LD)
    c, s = np.cos(LD(theta)), np.sin(LD(theta))
    U[p, p] = U[q, q] = c; U[p, q] = s; U[q, p] = -s
    return U


def rotate_integrals(h, eri, U):
    U, h, eri = np.asarray(U, LD), np.asarray(h, LD), np.asarray(eri, LD)
    h2 = np.einsum("aP,bQ,ab->PQ", U, U, h)
    t = np.einsum("aP,abcd->Pbcd", U, eri)
    t = np.einsum("bQ,Pbcd->PQcd", U, t)
    t = np.einsum("cR,PQcd->PQRd", U, t)
    return h2, np.einsum("dS,PQRd->PQRS", U, t)


def energy_on(h, eri, D, G):
    """sum h D + 1/2 sum (pr|qs) G[p,q,r,s] in longdouble"""
    return np.sum(np.asarray(h, LD) * np.asarray(D, LD)) + LD(0.5) * np.sum(np.asarray(eri, LD) * np.asarray(G, LD).transpose(0, 2, 1, 3))


def energy(h, eri, D, G, U=None):
    if U is None:
        return energy_on(h, eri, D, G)
    return energy_on(*rotate_integrals(h, eri, U), D, G)


def _patterns(T, W, pq):
    """[(m, M_S)] over the non-empty slot sets S: M_S[a_S..., P_S...] = sum over the other slots of T[a_S, rest] W[P_S, rest]"""
    k, out = T.ndim, []
    for m in range(1, k + 1):
        for S in combinations(range(k), m):
            Ts, Ws = T, W
            for ax in S:
                Ts, Ws = np.take(Ts, pq, axis=ax), np.take(Ws, pq, axis=ax)
            free = [ax for ax in range(k) if ax not in S]
            out.append((m, np.tensordot(Ts.astype(LD), Ws.astype(LD), axes=(free, free))))
    return out


def _eval_patterns(pats, V):
    tot = LD(0)
    for m, M in pats:
        sub = "abcd"[:m] + "ABCD"[:m] + "".join("," + x + y for x, y in zip("abcd"[:m], "ABCD"[:m]))
        tot = tot + np.einsum(sub + "->", M, *([V] * m))
    return tot


def plane_samples(h, eri, D, G, p, q, angles=ANGLES):
    """E(theta_j) - E(0) at theta_j = 2 pi j / angles along the plane rotation (p, q)"""
    pq = [p, q]
    pats1 = _patterns(np.asarray(h), np.asarray(D), pq)
    pats2 = _patterns(np.asarray(eri), np.asarray(G).transpose(0, 2, 1, 3), pq)
    out = []
    for j in range(angles):
        th = 2 * PI * LD(j) / LD(angles) if j else LD(0)
        c, s = np.cos(th), np.sin(th)
        V = np.array([[c - 1, s], [-s, c - 1]], LD)
        out.append(_eval_patterns(pats1, V) + LD(0.5) * _eval_patterns(pats2, V))
    return out


def full_samples(h, eri, D, G, p, q, angles=ANGLES):
    """E(theta_j) with the integrals transformed by einsum"""
    n = np.asarray(h).shape[0]
    return [energy(h, eri, D, G, plane_rotation(n, p, q, 2 * PI * LD(j) / LD(angles))) for j in range(angles)]


def fourier_derivatives(samples):
    """(E'(0), E''(0)) of the trigonometric polynomial of degree <= 4 through its samples at 2 pi j / len(samples), len >= 9"""
    N = len(samples)
    assert N >= 9
    E = np.asarray(samples, LD)
    th = 2 * PI * np.arange(N, dtype=LD) / LD(N)
    d1 = d2 = LD(0)
    for k in range(1, 5):
        a_k = LD(2) / LD(N) * np.sum(E * np.cos(k * th))
        b_k = LD(2) / LD(N) * np.sum(E * np.sin(k * th))
        d1 = d1 + k * b_k
        d2 = d2 - k * k * a_k
    return d1, d2


def derivatives(h, eri, D, G, pairs=None, full=False):
    """{(p, q): (E'(0), E''(0))} along K_pq for the pairs (default: every p != q)"""
    n = np.asarray(h).shape[0]
    if pairs is None:
        pairs = [(p, q) for p in range(n) for q in range(n) if p != q]
    fn = full_samples if full else plane_samples
    return {(p, q): fourier_derivatives(fn(h, eri, D, G, p, q)) for p, q in pairs}


def all_pair_derivatives(h, eri, D, G):
    """(d1[p, q], d2[p, q]) = (E'(0), E''(0)) along K_pq for every pair at once (diagonals 0): plane_samples' expansion with the pair
    (p, q) kept as two free indices.  A pattern with V on the slots S, the old indices a_S and the new indices P_S each chosen among
    {p, q}, is one einsum over the remaining slots whose result is a matrix over (p, q); its weight at angle j is the product of the
    chosen entries of V_j.  Same algebra, same samples, same Fourier sums; O(n^5) in all where plane_samples is O(n^3) per pair."""
    from itertools import product
    n = np.asarray(h).shape[0]
    th = 2 * PI * np.arange(ANGLES, dtype=LD) / LD(ANGLES)
    c, s = np.cos(th), np.sin(th)
    V = np.empty((ANGLES, 2, 2), LD)
    V[:, 0, 0] = V[:, 1, 1] = c - 1; V[:, 0, 1] = s; V[:, 1, 0] = -s
    E = np.zeros((ANGLES, n, n), LD)
    for T, W, wgt in ((np.asarray(h, LD), np.asarray(D, LD), LD(1)),
                      (np.asarray(eri, LD), np.ascontiguousarray(np.asarray(G, LD).transpose(0, 2, 1, 3)), LD(0.5))):
        k = T.ndim
        for m in range(1, k + 1):
            for S in combinations(range(k), m):
                for ca in product((0, 1), repeat=m):
                    for cp in product((0, 1), repeat=m):
                        tl, wl = list("rstu"[:k]), list("rstu"[:k])
                        for i, ax in enumerate(S):
                            tl[ax], wl[ax] = "pq"[ca[i]], "pq"[cp[i]]
                        out = "".join(x for x in "pq" if x in tl or x in wl)
                        X = np.einsum("".join(tl) + "," + "".join(wl) + "->" + out, T, W)
                        X = X if out == "pq" else X[:, None] if out == "p" else X[None, :]
                        coef = np.ones(ANGLES, LD)
                        for i in range(m):
                            coef = coef * V[:, ca[i], cp[i]]
                        E = E + wgt * coef[:, None, None] * X[None]
    d1, d2 = np.zeros((n, n), LD), np.zeros((n, n), LD)
    for kk in range(1, 5):
        a_k = LD(2) / LD(ANGLES) * np.tensordot(np.cos(kk * th), E, axes=(0, 0))
        b_k = LD(2) / LD(ANGLES) * np.tensordot(np.sin(kk * th), E, axes=(0, 0))
        d1, d2 = d1 + kk * b_k, d2 - kk * kk * a_k
    np.fill_diagonal(d1, 0); np.fill_diagonal(d2, 0)
    return d1, d2


# ------------------------------------------------------------------------------------------------------- the Fock matrix and the bounds
def fock_literal(h, eri, D, G):
    """F[a,P] = sum_r h[a,r] D[P,r] + sum_qrs (ar|qs) G[P,q,r,s] in longdouble, whatever the arrays"""
    n = np.asarray(h).shape[0]
    A = np.asarray(eri, LD).transpose(0, 2, 1, 3).reshape(n, n ** 3)          # [a, (q, r, s)]
    B = np.asarray(G, LD).reshape(n, n ** 3)                                  # [P, (q, r, s)]
    return np.asarray(h, LD) @ np.asarray(D, LD).T + A @ B.T


def fock_entries(h, eri, D, G, entries):
    """the same for a list of (a, P), each a longdouble sum of its own (64 orbitals: no dense longdouble copy)"""
    out = {}
    for a, P in entries:
        one = np.sum(np.asarray(h[a], LD) * np.asarray(D[P], LD))
        two = np.sum(np.asarray(eri[a], LD).transpose(1, 0, 2) * np.asarray(G[P], LD))
        out[(a, P)] = one + two
    return out


def fock_abs(h, eri, D, G):
    """sum of |terms| of every F[a,P] (double precision: a bound's scale)"""
    n = np.asarray(h).shape[0]
    A = np.abs(np.asarray(eri, float)).transpose(0, 2, 1, 3).reshape(n, n ** 3)
    return np.abs(h) @ np.abs(D).T + A @ np.abs(np.asarray(G, float)).reshape(n, n ** 3).T


def fock_terms(n):
    return n ** 3 + n


def fock_bound(n, sum_abs):
    """|F - exact| <= (norb^3 + norb + 2) 2^-53 sum|terms|: a double-precision sum of that many products in any order"""
    return (fock_terms(n) + 2) * U53 * sum_abs


def hdiag_terms(n):
    """hdiag[p,q] as one sum: the 2 (norb^3 + norb) terms of F[p,p] and F[q,q], three one-body products, 3 norb^2 terms per Y sum"""
    return 2 * fock_terms(n) + 9 * n * n + 3


def _y_abs(ah, ae, aD, aG, x, P, y, Q):
    one = ah[x, y] * aD[P, Q]
    a1 = np.sum(ae[x, y] * aG[P, :, Q, :])
    a2 = np.sum(ae[x, :, y, :] * (aG[P, Q] + aG[P, :, :, Q].T))
    return 2.0 * (one + a1 + a2)


def hdiag_abs(h, eri, D, G, pairs, fabs=None):
    """{(p, q): sum of |terms| of hdiag[p,q]} with every term of F[p,p], F[q,q] and of the three Y sums counted at its weight"""
    ah, ae, aD, aG = (np.abs(np.asarray(x, float)) for x in (h, eri, D, G))
    fabs = fock_abs(h, eri, D, G) if fabs is None else fabs
    return {(p, q): 2.0 * (fabs[p, p] + fabs[q, q]) + _y_abs(ah, ae, aD, aG, p, q, p, q) + _y_abs(ah, ae, aD, aG, q, p, q, p)
            + 2.0 * _y_abs(ah, ae, aD, aG, p, q, q, p) for p, q in pairs}


def hdiag_bound(n, sum_abs):
    return (hdiag_terms(n) + 2) * U53 * sum_abs


def gradient_bound(n, fabs, p, q):
    """twice the sum of the bounds of F[p,q] and F[q,p]"""
    return 2.0 * (fock_bound(n, fabs[p, q]) + fock_bound(n, fabs[q, p]))


# ------------------------------------------------------------------------------------- wavefunctions, through the other checkers
def dense_hamiltonian(h, eri, core=0.0):
    """proposal_checker's second-quantised Hamiltonian on dense integrals: spin orbital P = p (up) or norb + p (dn)"""
    from tests import proposal_checker as PC

    class DenseH(PC.Hamiltonian):
        def __init__(self):
            self.norb, self.const = int(np.asarray(h).shape[0]), float(core)
            self.h1, self.h2 = np.asarray(h, float), np.asarray(eri, float)

        def t(self, P, Q):
            n = self.norb
            return float(self.h1[P % n, Q % n]) if P // n == Q // n else 0.0

        def v(self, P, Q, R, S):
            n = self.norb
            return float(self.h2[P % n, Q % n, R % n, S % n]) if P // n == Q // n and R // n == S // n else 0.0

    return DenseH()


def complete_space(norb, nup, ndn):
    """every determinant (up, dn) of nup + ndn electrons in norb orbitals"""
    ups = [sum(1 << k for k in c) for c in combinations(range(norb), nup)]
    dns = [sum(1 << k for k in c) for c in combinations(range(norb), ndn)]
    return [(a, b) for a in ups for b in dns]


def hamiltonian_matrix(H, dets):
    return np.array([[H.element(ju, jd, iu, id_)[0] for (ju, jd) in dets] for (iu, id_) in dets])


def density_matrices(dets, coeffs, norb):
    """(D, G) as arrays from rdm_checker and rdm2_checker: D[p, r] spin-summed, G[p, q, r, s] spin-free"""
    from tests import rdm_checker as RC
    from tests import rdm2_checker as R2
    D = np.array(RC.one_rdm(dets, coeffs, norb).matrix())
    two = R2.two_rdm(dets, coeffs, norb)
    G = np.zeros((norb,) * 4)
    for idx in np.ndindex(*G.shape):
        G[idx] = two.spin_free(idx)[0]
    return D, G


def energy_bound(h, eri, D, G, U, const_n2=0.0):
    """delta: the bound on one fixed-coefficient energy  E = sum h' D + 1/2 sum (pr|qs)' G + const n2  formed in double precision from
    integrals rotated in double precision by U.  Entries: rotate_checker's bound, 4 (norb + 1) 2^-53 S for a two-body entry and
    2 (norb + 1) 2^-53 S for a one-body entry, S the transformation of |integrals| by |U|; they enter E weighted by |G| / 2 and |D|.
    The sum itself: norb^4 + norb^2 + 2 terms in any order, (that many) 2^-53 sum |terms| with |terms| <= S |D| or S |G| / 2."""
    n = np.asarray(h).shape[0]
    S1, S2 = rotate_integrals(np.abs(np.asarray(h, float)), np.abs(np.asarray(eri, float)), np.abs(np.asarray(U, float)))
    m1 = float(np.sum(np.asarray(S1, float) * np.abs(D)))
    m2 = 0.5 * float(np.sum(np.asarray(S2, float) * np.abs(np.asarray(G, float)).transpose(0, 2, 1, 3)))
    return (2 * (n + 1) * m1 + 4 * (n + 1) * m2) * U53 + (n ** 4 + n ** 2 + 2) * U53 * (m1 + m2 + abs(const_n2))
