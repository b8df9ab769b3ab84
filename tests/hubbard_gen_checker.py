"""An independent, plain model of the real-space Hubbard connection generator ('hubbard2'), on top of tests/proposal_checker.py
(HubbardH, second quantisation on bit strings, rounding_bound) and of nothing from oracle/ or the HIP library.

The lattice is geometry here, not a neighbour table: site s (0-based) sits at x = s mod l_x, y = s div l_x; LEFT, RIGHT, UP, DOWN are
(x - 1, y), (x + 1, y), (x, y + 1), (x, y - 1), wrapped when periodic; a direction is allowed when it leads to another site of the
lattice (an open edge has none; a periodic direction of length 1 leads back to the site itself; length 2 is refused, as the library
refuses it).  The generator's order: sites ascending, at each site the up electron before the dn electron, per electron the four
directions in that order; a hop exists when the neighbour is allowed and empty in that spin's string."""
import itertools
import math
import random

import numpy as np

from tests import proposal_checker as PC

DIRECTIONS = ((-1, 0), (1, 0), (0, 1), (0, -1))          # LEFT, RIGHT, UP, DOWN
U53 = 2.0 ** -53


def neighbour(l_x, l_y, pbc, s, k):
    """the site in direction k of site s (both 0-based), or None when not allowed"""
    assert not pbc or (l_x != 2 and l_y != 2)
    x, y = s % l_x, s // l_x
    nx, ny = x + DIRECTIONS[k][0], y + DIRECTIONS[k][1]
    if pbc:
        nx, ny = nx % l_x, ny % l_y
    if not (0 <= nx < l_x and 0 <= ny < l_y) or (nx, ny) == (x, y):
        return None
    return ny * l_x + nx


class Lattice(PC.HubbardH):
    """PC.HubbardH with its geometry kept; a direction of length 1 (a chain), which square_lattice_bonds refuses when periodic, gets
    its bonds from neighbour() instead"""

    def __init__(self, l_x, l_y, pbc, t, U):
        self.l_x, self.l_y, self.pbc = l_x, l_y, bool(pbc)
        if pbc and (l_x == 1 or l_y == 1):
            self.norb, self.t_hop, self.U = l_x * l_y, float(t), float(U)
            nb = {(s, neighbour(l_x, l_y, pbc, s, k)) for s in range(self.norb) for k in range(4)}
            self.bonds = sorted({tuple(sorted(b)) for b in nb if b[1] is not None})
            self.bonded = set(self.bonds) | {(b, a) for a, b in self.bonds}
            self.nbrs = {s: sorted(b for a, b in self.bonded if a == s) for s in range(self.norb)}
        else:
            PC.HubbardH.__init__(self, l_x, l_y, pbc, t, U)


def hops(H, up, dn):
    """[(site, spin (0 up, 1 dn), direction, child)] in the generator's order"""
    out = []
    for s in range(H.norb):
        for sp, cfg in ((0, up), (1, dn)):
            if not cfg >> s & 1:
                continue
            for k in range(4):
                nb = neighbour(H.l_x, H.l_y, H.pbc, s, k)
                if nb is None or cfg >> nb & 1:
                    continue
                nc = cfg ^ (1 << s) ^ (1 << nb)
                out.append((s, sp, k, (nc, dn) if sp == 0 else (up, nc)))
    return out


def children(H, up, dn):
    return [h[3] for h in hops(H, up, dn)]


def all_determinants(norb, nup, ndn):
    strings = lambda n: [sum(1 << o for o in c) for c in itertools.combinations(range(norb), n)]
    return sorted((u, d) for u in strings(nup) for d in strings(ndn))


def connections(H, refs, coeffs, eps, diag_mode):
    """what the generator must return, by brute force: per reference determinant with c != 0 its own slot (H_ii c in diag_mode 1,
    else 0; e_mix_den = c) and every hop child with |H c| > eps (strict), summed per determinant.
    Returns {det: (num, den, n_terms, sum|terms|)} (a determinant's own slot counts the terms of its H_ii); diag_mode 2 (raw) returns
    the list [(det, num, source index)] in generation order, the source's own slot first."""
    raw, acc = [], {}
    for i, ((u, d), c) in enumerate(zip(refs, coeffs)):
        if c == 0.0:
            continue
        hd, hn, hs = H.element(u, d, u, d) if diag_mode == 1 else (0.0, 1, 0.0)      # H_ii is itself a sum of hn terms
        raw.append(((u, d), hd * c, float(i)))
        ent = [((u, d), hd * c, c, max(hn, 1), hs * abs(c))]
        for ch in children(H, u, d):
            h, n, _ = H.element(u, d, ch[0], ch[1])
            if n and abs(h * c) > eps:               # (t = 0: no term, no hop)
                raw.append((ch, h * c, float(i)))
                ent.append((ch, h * c, 0.0, 1, abs(h * c)))
        for det, num, den, n, sa in ent:
            a = acc.setdefault(det, [0.0, 0.0, 0, 0.0])
            a[0] += num; a[1] += den; a[2] += n; a[3] += sa
    return raw if diag_mode == 2 else {k: tuple(v) for k, v in acc.items()}


def pt2(H, var, coeffs, e_var, eps):
    """explicit Epstein-Nesbet sum over the connected determinants a outside var of (sum_i H_ai c_i)^2 / (E_var - H_aa), the inner sum
    over |H_ai c_i| > eps.  Returns (delta_e, determinants outside, determinants visited (var's own slots included), bound): the
    bound propagates rounding_bound of every inner sum and of H_aa through the square, the difference and the quotient, plus the
    outer sum's own rounding."""
    var = [(int(a), int(b)) for a, b in var]
    con = connections(H, var, list(coeffs), eps, 0)
    inside = set(var)
    terms, bounds = [], []
    for det, (x, _, n, sa) in con.items():
        if det in inside:
            continue
        haa, hn, hs = H.element(det[0], det[1], det[0], det[1])
        den = e_var - haa
        t = x * x / den
        bx, bd = PC.rounding_bound(n, sa), PC.rounding_bound(max(hn, 1), hs) + U53 * (abs(e_var) + abs(haa))
        terms.append(t)
        bounds.append((2.0 * abs(x) * bx + bx * bx) / abs(den) + abs(t) * (bd / abs(den) + 3.0 * U53))
    bound = math.fsum(bounds) + len(terms) * U53 * math.fsum(abs(t) for t in terms)
    return math.fsum(terms), len(terms), len(con), bound


def breadth_first(H, start, n_levels):
    """the start determinant and everything within n_levels hops, sorted"""
    seen, frontier = {start}, [start]
    for _ in range(n_levels):
        nxt = []
        for u, d in frontier:
            for ch in children(H, u, d):
                if ch not in seen:
                    seen.add(ch); nxt.append(ch)
        frontier = nxt
    return sorted(seen)


def dense(H, dets):
    """the matrix of H among dets: the diagonal and, per determinant, the elements to its hop children that lie in dets
    (that the children are all there is to a row is what the self-test checks, against every pair)"""
    idx = {d: i for i, d in enumerate(dets)}
    A = np.zeros((len(dets), len(dets)))
    for i, (u, d) in enumerate(dets):
        A[i, i] = H.element(u, d, u, d)[0]
        for ch in children(H, u, d):
            j = idx.get(ch)
            if j is not None:
                A[j, i] = H.element(u, d, ch[0], ch[1])[0]
    return A


def ground_energy(H, dets):
    return float(np.linalg.eigvalsh(dense(H, dets))[0])


def neel(l_x, l_y, nup, ndn):
    """the start determinant of the walk: up on x + y even first, dn on x + y odd first"""
    sites = range(l_x * l_y)
    even = [q for q in sites if ((q % l_x) + (q // l_x)) % 2 == 0]
    odd = [q for q in sites if ((q % l_x) + (q // l_x)) % 2 == 1]
    return sum(1 << q for q in (even + odd)[:nup]), sum(1 << q for q in (odd + even)[:ndn])


def conn_case(l_x, l_y, pbc, t, U, seed):
    """the fixture of the connection test: 40 random reference determinants of (2,2); |H| = |t| throughout, so |H c| > eps cuts on
    |c|: coefficients on both sides of the cut (more than 8 sources on each), one zero (emits nothing, its own slot included) and one
    exact tie (|H c| == eps: its hops dropped, its own slot kept)"""
    H = Lattice(l_x, l_y, pbc, t, U)
    rng = random.Random(seed)
    refs = rng.sample(all_determinants(l_x * l_y, 2, 2), 40)
    c_tie = 0.03
    eps = abs(H.t_hop * c_tie)
    coeffs = [rng.choice((-1, 1)) * 10.0 ** rng.uniform(-2.5, -0.5) for _ in refs]
    coeffs[7], coeffs[19] = 0.0, -c_tie
    assert abs(-H.t_hop * coeffs[19]) == eps
    above = sum(1 for c in coeffs if abs(H.t_hop * c) > eps)
    below = sum(1 for c in coeffs if c != 0.0 and not abs(H.t_hop * c) > eps)
    assert above > 8 and below > 8, (above, below)
    return H, refs, coeffs, eps
