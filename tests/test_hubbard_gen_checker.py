"""tests/hubbard_gen_checker.py against itself and against tests/proposal_checker.py, on the CPU: the hop list is the whole
off-diagonal row (every pair of determinants is asked), the two-site model has its textbook ground energy, and the fixture of the
GPU connection test has sources on both sides of the screen."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hubbard_gen_checker as HG       # noqa: E402

T_HOP, U = 0.75, 3.0


def _popcount(a):
    a = a.copy(); n = np.zeros(a.shape, np.int64)
    while a.any():
        n += (a & np.uint64(1)).astype(np.int64); a >>= np.uint64(1)
    return n


@pytest.mark.parametrize("l_x,l_y,pbc", [(3, 3, True), (4, 3, False)], ids=["3x3_periodic", "4x3_open"])
def test_hop_children_are_the_off_diagonal_row(l_x, l_y, pbc):
    """every ordered pair I != J of (2,2) determinants: <J|H|I> has a term exactly when J is a hop child of I, and then the
    value the checker's connection list uses.  Three classes, by the number of spin orbitals of I that J lacks:
    one -- every pair is evaluated (the spectators enter through v);
    two -- Hamiltonian.terms can only annihilate the two orbitals J lacks and create the two I lacks, so whether it lists a term
    depends on those four orbitals alone (the other electrons give signs, and terms are listed, not summed): one pair is
    evaluated for every distinct (removed, added) combination that occurs, and the combination decides for all pairs that share it;
    more -- counted, not evaluated: terms returns nothing for them before it looks at t or v."""
    H = HG.Lattice(l_x, l_y, pbc, T_HOP, U)
    n = H.norb
    dets = HG.all_determinants(n, 2, 2)
    states = np.array([H.state(u, d) for u, d in dets], np.uint64)
    singles = doubles = skipped = with_terms = 0
    combos = {}                                              # (removed, added) -> one pair (i, j) that has it
    value = {}                                               # (i, j) -> the hop's element
    for i, (u, d) in enumerate(dets):
        kids = HG.children(H, u, d)
        assert len(kids) == len(set(kids)) and (u, d) not in kids
        kidset = set(kids)
        rem = states[i] & ~states
        moved = _popcount(rem)                               # spin orbitals of I that J lacks
        one, two = np.nonzero(moved == 1)[0], np.nonzero(moved == 2)[0]
        skipped += len(dets) - 1 - len(one) - len(two)
        for j in one.tolist():
            tm = H.terms(u, d, dets[j][0], dets[j][1])
            singles += 1
            if dets[j] in kidset:
                assert len(tm) == 1 and abs(tm[0]) == T_HOP, ((u, d), dets[j], tm)
                value[(i, j)] = tm[0]
                with_terms += 1
            else:
                assert tm == [], ((u, d), dets[j], tm)
        assert kidset <= {dets[j] for j in one.tolist()}
        doubles += len(two)
        add = states[two] & ~states[i]
        cr, first = np.unique(np.stack((rem[two], add), axis=1), axis=0, return_index=True)
        for (r, a), k in zip(cr.tolist(), first.tolist()):
            combos.setdefault((r, a), (i, int(two[k])))
    assert all(value[(j, i)] == v for (i, j), v in value.items())          # symmetric: (j, i) is a pair of its own above
    for (r, a), (i, j) in combos.items():
        assert PC._pop(r) == PC._pop(a) == 2 and states[i] & ~states[j] == r and states[j] & ~states[i] == a
        assert H.terms(dets[i][0], dets[i][1], dets[j][0], dets[j][1]) == [], (dets[i], dets[j])
    far = dets[0], dets[-1]
    assert PC._pop(H.state(*far[0]) & ~H.state(*far[1])) > 2 and H.terms(*far[0], *far[1]) == []
    print("%dx%d %s (2,2): %d determinants; pairs one orbital apart %d (all evaluated, %d hops), two apart %d (%d combinations evaluated), further %d"
          % (l_x, l_y, "periodic" if pbc else "open", len(dets), singles, with_terms, doubles, len(combos), skipped))
    assert singles + doubles + skipped == len(dets) * (len(dets) - 1) and len(combos) > 1000
    # each bond carries each electron of a string across when the far site is empty: counted from the bonds, not from hops()
    want = sum(1 for u, d in dets for a, b in H.bonded for cfg in (u, d) if cfg >> a & 1 and not cfg >> b & 1)
    assert with_terms == want > 0


def test_hop_order_and_edges():
    H = HG.Lattice(4, 3, False, T_HOP, U)
    # site 0 (a corner): no LEFT, no DOWN; RIGHT is site 1, UP is site 4
    assert [HG.neighbour(4, 3, False, 0, k) for k in range(4)] == [None, 1, 4, None]
    assert [HG.neighbour(4, 3, True, 0, k) for k in range(4)] == [3, 1, 4, 8]
    assert [HG.neighbour(6, 1, True, 0, k) for k in range(4)] == [5, 1, None, None]
    up, dn = 0b100001, 0b000001                    # up on sites 0 and 5, dn on site 0
    got = [(s, sp, k) for s, sp, k, _ in HG.hops(H, up, dn)]
    assert got == [(0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (5, 0, 0), (5, 0, 1), (5, 0, 2), (5, 0, 3)]
    ring = HG.Lattice(6, 1, True, T_HOP, U)
    assert ring.bonds == [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert HG.Lattice(3, 3, True, T_HOP, U).bonds == PC.square_lattice_bonds(3, 3, True)


def test_two_site_ground_energy():
    """one up and one dn electron on two sites: E0 = (U - sqrt(U^2 + 16 t^2)) / 2"""
    for t, u in ((1.0, 4.0), (0.75, 3.0), (1.0, 0.0), (0.3, 12.0)):
        H = HG.Lattice(2, 1, False, t, u)
        dets = HG.all_determinants(2, 1, 1)
        assert len(dets) == 4
        e0 = HG.ground_energy(H, dets)
        want = (u - math.sqrt(u * u + 16.0 * t * t)) / 2.0
        assert abs(e0 - want) <= 1e-13 * max(1.0, abs(want)), (t, u, e0, want)


@pytest.mark.parametrize("l_x,l_y,pbc,seed", [(4, 3, False, 17), (3, 3, True, 18)], ids=["4x3_open", "3x3_periodic"])
def test_connection_fixture_cuts_on_both_sides(l_x, l_y, pbc, seed):
    H, refs, coeffs, eps = HG.conn_case(l_x, l_y, pbc, T_HOP, U, seed)        # asserts more than 8 sources on each side itself
    assert len(refs) == len(set(refs)) == 40 and coeffs[7] == 0.0 and abs(H.t_hop * coeffs[19]) == eps
    raw = HG.connections(H, refs, coeffs, eps, 2)
    assert not any(r[2] == 7.0 for r in raw)                                   # c = 0: nothing, its own slot included
    assert [r[0] for r in raw if r[2] == 19.0] == [refs[19]]                   # the tie keeps its own slot and nothing else
    merged = HG.connections(H, refs, coeffs, eps, 1)
    assert set(merged) == {r[0] for r in raw} and sum(v[2] for v in merged.values()) >= len(raw)
    if not pbc:
        assert any(len(HG.hops(H, u, d)) < 16 for u, d in refs)               # edges: fewer than 4 hops per electron


def test_pt2_and_breadth_first_are_consistent():
    H = HG.Lattice(3, 3, True, T_HOP, U)
    start = HG.neel(3, 3, 2, 2)
    lv = [HG.breadth_first(H, start, k) for k in range(8)]
    assert [len(x) for x in lv][:2] == [1, 1 + len(HG.children(H, *start))]
    assert all(set(a) <= set(b) for a, b in zip(lv, lv[1:])) and len(lv[-1]) == 1296
    var = lv[1]
    w, X = np.linalg.eigh(HG.dense(H, var))
    de, n_out, n_vis, bound = HG.pt2(H, var, X[:, 0].tolist(), float(w[0]), 1e-12)
    # (a coefficient that is zero by symmetry brings nothing in, so the visited set may be smaller than the second level)
    assert de < 0 and 10 < n_out <= len(lv[2]) - len(lv[1]) and n_out + len(var) >= n_vis > n_out and 0 < bound < 1e-12 * abs(de)
