"""An independent yardstick for the one-index transformation and the orbital Hessian-vector product.  Nothing here comes from sqmc_amd/
or oracle/, and sigma takes nothing from the library's formula: it is read off the energy itself.

Conventions are orbopt_checker's (0-based orbitals): h[p, r]; eri[p, r, q, s] = (pr|qs); D[p, r]; spin-free G[p, q, r, s];
E = sum h D + 1/2 sum (pr|qs) G[p,q,r,s]; a rotation U defines new_P = sum_k U[k, P] old_k and E(U) is the energy of the FIXED D, G on
the rotated integrals (orbopt_checker.energy).  K_pq = e_p e_q^T - e_q e_p^T.

sigma from energies.  E(U) is a polynomial of degree 4 in the entries of U.  The second-order Taylor coefficient Q(X) of E(exp(theta X))
depends on exp only up to theta^2, so it is the theta^2 coefficient of  P(theta) = E(I + theta X + theta^2 X^2 / 2),  a polynomial of
degree 8 in theta.  Half its second derivative at 0 comes from nine samples at theta = j / 4, j = -4 .. 4, by the nine-point central
formula, which is exact for polynomials up to degree 9: no step size to choose and no truncation error (the nodes are exact in binary,
|theta| <= 1 keeps the high powers small).  Q is a quadratic form in X, so by polarisation
    sigma(kappa) . Y = d2/ds dt E(exp(s kappa + t Y)) at 0 = Q(kappa + Y) - Q(kappa) - Q(Y),      sigma(kappa)[p, q] = sigma(kappa) . K_pq.

one_index_literal is this module's own statement of the one-index transformation, and sigma_literal a second, literal statement of
sigma in longdouble: it is used only at the sizes where the energy route is too slow, and test_orbhess_checker pins it to the energy
route at the small ones.  The *_abs functions are the sums of absolute values behind the rounding bounds."""
import numpy as np

from tests import orbopt_checker as OC

LD = np.longdouble
U53 = 2.0 ** -53
# second derivative at 0 from samples at -4h .. 4h, times h^2: exact up to degree 9
_W9 = [LD(-1) / LD(560), LD(8) / LD(315), LD(-1) / LD(5), LD(8) / LD(5), LD(-205) / LD(72), LD(8) / LD(5), LD(-1) / LD(5), LD(8) / LD(315), LD(-1) / LD(560)]
_STEP = LD(1) / LD(4)


def K(n, p, q):
    k = np.zeros((n, n), LD)
    k[p, q], k[q, p] = 1, -1
    return k


def random_kappa(n, seed, antisymmetric=True):
    k = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))
    return np.triu(k, 1) - np.triu(k, 1).T if antisymmetric else k


# ---------------------------------------------------------------------------------------------------------------- sigma from the energy
def second_order(h, eri, D, G, X):
    """Q(X): the theta^2 coefficient of E(I + theta X + theta^2 X^2 / 2)"""
    X = np.asarray(X, LD)
    n = X.shape[0]
    X2 = X @ X / LD(2)
    tot = LD(0)
    for j, w in zip(range(-4, 5), _W9):
        th = LD(j) * _STEP
        tot = tot + w * OC.energy(h, eri, D, G, np.eye(n, dtype=LD) + th * X + th * th * X2)
    return tot / (_STEP * _STEP) / LD(2)


def sigma_dot(h, eri, D, G, kappa, Y):
    """sigma(kappa) . Y"""
    kappa, Y = np.asarray(kappa, LD), np.asarray(Y, LD)
    return second_order(h, eri, D, G, kappa + Y) - second_order(h, eri, D, G, kappa) - second_order(h, eri, D, G, Y)


def sigma_from_energy(h, eri, D, G, kappa):
    """sigma(kappa)[p, q] for every pair, antisymmetric with a zero diagonal by construction (K_qp = -K_pq)"""
    n = np.asarray(h).shape[0]
    qk = second_order(h, eri, D, G, kappa)
    out = np.zeros((n, n), LD)
    for p in range(n):
        for q in range(p + 1, n):
            Y = K(n, p, q)
            out[p, q] = second_order(h, eri, D, G, np.asarray(kappa, LD) + Y) - qk - second_order(h, eri, D, G, Y)
            out[q, p] = -out[p, q]
    return out


def hessian_matrix(h, eri, D, G, pairs):
    """the dense Hessian over the pair coordinates: H[i, j] = sigma(K_pairs[j]) . K_pairs[i], in double"""
    n = np.asarray(h).shape[0]
    Ks = [K(n, p, q) for p, q in pairs]
    q1 = [second_order(h, eri, D, G, k) for k in Ks]
    H = np.zeros((len(pairs), len(pairs)))
    for i in range(len(pairs)):
        H[i, i] = float(2 * q1[i])
        for j in range(i):
            H[i, j] = H[j, i] = float(second_order(h, eri, D, G, Ks[i] + Ks[j]) - q1[i] - q1[j])
    return H


# --------------------------------------------------------------------------------------------------------- the literal statements
def one_index_literal(h, eri, kappa, dtype=LD):
    """h~[P,Q] = sum_a k[a,P] h[a,Q] + sum_b k[b,Q] h[P,b];  (PQ|RS)~ = the same on each of the four indices"""
    k, h, eri = np.asarray(kappa, dtype), np.asarray(h, dtype), np.asarray(eri, dtype)
    n = k.shape[0]
    ht = k.T @ h + h @ k
    et = np.tensordot(k, eri, axes=(0, 0))                                                      # [P, Q, R, S] <- k[a,P] eri[a,Q,R,S]
    et = et + np.tensordot(k, eri, axes=(0, 1)).transpose(1, 0, 2, 3)                           # k[b,Q] eri[P,b,R,S]
    et = et + np.tensordot(k, eri, axes=(0, 2)).transpose(1, 2, 0, 3)                           # k[c,R] eri[P,Q,c,S]
    et = et + np.tensordot(eri, k, axes=(3, 0))                                                 # eri[P,Q,R,d] k[d,S]
    assert et.shape == (n,) * 4
    return ht, et


def one_index_entry(eri, kappa, P, Q, R, S):
    """(PQ|RS)~ alone, four longdouble sums of norb products (64 orbitals: no dense longdouble tensor)"""
    k = np.asarray(kappa, LD)
    return (np.sum(k[:, P] * np.asarray(eri[:, Q, R, S], LD)) + np.sum(k[:, Q] * np.asarray(eri[P, :, R, S], LD))
            + np.sum(k[:, R] * np.asarray(eri[P, Q, :, S], LD)) + np.sum(k[:, S] * np.asarray(eri[P, Q, R, :], LD)))


def one_index_abs(h, eri, kappa):
    """the same sums with every factor replaced by its absolute value (double precision: a bound's scale)"""
    return one_index_literal(np.abs(np.asarray(h, float)), np.abs(np.asarray(eri, float)), np.abs(np.asarray(kappa, float)), float)


def one_index_bound(n, abs_one, abs_two):
    """(bound on h~, bound on (PQ|RS)~): a double-precision sum of 2 norb or 4 norb products in any order, (terms + 2) 2^-53 sum|terms|"""
    return (2 * n + 2) * U53 * abs_one, (4 * n + 2) * U53 * abs_two


def sigma_literal(h, eri, D, G, kappa):
    """sigma = 2 (F~ - F~^T) + 1/2 (kappa g - g kappa) in longdouble, F~ = orbopt_checker.fock_literal on the literal transform"""
    k = np.asarray(kappa, LD)
    ht, et = one_index_literal(h, eri, k)
    Ft = OC.fock_literal(ht, et, D, G)
    F = OC.fock_literal(h, eri, D, G)
    g = LD(2) * (F - F.T)
    return LD(2) * (Ft - Ft.T) + (k @ g - g @ k) / LD(2)


def sigma_literal_entries(h, eri, D, G, kappa, pairs, g):
    """{(p, q): sigma[p, q]} for a list of pairs, each Fock entry a longdouble sum of its own (64 orbitals: no dense longdouble
    tensor); g: the gradient at kappa = 0 as the caller has it"""
    k, g = np.asarray(kappa, LD), np.asarray(g, LD)
    hl, Dl = np.asarray(h, LD), np.asarray(D, LD)
    ht = k.T @ hl + hl @ k
    rows = {}

    def fock_row(a):
        """et[a, :, :, :] and from it F~[a, P] for every P"""
        if a not in rows:
            ea = np.asarray(eri[a], LD)                                                         # [r, q, s] = (a r|q s)
            et = np.tensordot(k, ea, axes=(0, 0))                                               # [r', q, s] <- k[r,r'] (a r|q s)
            for x in range(k.shape[0]):                                                         # sum_x k[x,a] (x r|q s)
                et = et + k[x, a] * np.asarray(eri[x], LD)
            et = et + np.tensordot(k, ea, axes=(0, 1)).transpose(1, 0, 2)                       # k[q,q'] (a r|q s)
            et = et + np.tensordot(ea, k, axes=(2, 0))                                          # (a r|q s) k[s,s']
            GP = np.asarray(G, float)
            rows[a] = np.array([np.sum(ht[a] * Dl[P]) + np.sum(et.transpose(1, 0, 2) * GP[P].astype(LD)) for P in range(k.shape[0])], LD)
        return rows[a]
    out = {}
    for p, q in pairs:
        com = np.sum(k[p, :] * g[:, q]) - np.sum(g[p, :] * k[:, q])
        out[(p, q)] = LD(2) * (fock_row(p)[q] - fock_row(q)[p]) + com / LD(2)
    return out


# -------------------------------------------------------------------------------------------------------------------------- the bounds
def sigma_bound(n, h, eri, D, G, kappa, g, fabs0=None, g_factor=1.0):
    """|sigma_device - exact| entry by entry.  F~[a,P] is a sum of norb^3 + norb products whose integral factor is itself a sum of
    4 norb (2 norb) products: (norb^3 + norb + 2 + 4 norb + 2) 2^-53 times the sum with every factor in absolute value, in any
    order.  The commutator: two sums of norb products, (norb + 2) 2^-53 sum|terms| each, plus what the device's own g is off by
    (orbopt_checker.gradient_bound) carried through |kappa|; g_factor 2 when the checker's g is a double-precision sum too.  Four
    more roundings join the pieces."""
    ak, ag = np.abs(np.asarray(kappa, float)), np.abs(np.asarray(g, float))
    a1, a2 = one_index_abs(h, eri, kappa)
    s_abs = OC.fock_abs(a1, a2, D, G)
    b_ft = (n ** 3 + n + 2 + 4 * n + 2) * U53 * s_abs
    fabs0 = OC.fock_abs(h, eri, D, G) if fabs0 is None else fabs0
    dg = 2.0 * (OC.fock_bound(n, fabs0) + OC.fock_bound(n, fabs0).T)
    com_abs = ak @ ag + ag @ ak
    total_abs = 2.0 * (s_abs + s_abs.T) + 0.5 * com_abs
    return 2.0 * (b_ft + b_ft.T) + 0.5 * (n + 2) * U53 * com_abs + 0.5 * g_factor * (ak @ dg + dg @ ak) + 4 * U53 * total_abs
