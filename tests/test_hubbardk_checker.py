"""CPU checks of the plane-wave Hubbard model's conventions: HubbardKHost's orbital table against the checker's own, the full
spectrum of tests/hubbardk_checker.HubbardKH against the real-space model of tests/proposal_checker.py (the two are one operator in
two bases), the move's triples against the full row of H, and the deck grammar."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hubbardk_checker as HK          # noqa: E402

DECK = os.path.join(ROOT, "tests", "golden", "hubbardk4x3_i_walk")


@pytest.mark.parametrize("shape", [(3, 3), (4, 3), (4, 4), (8, 8), (6, 1)])
def test_host_k_table_is_the_checkers(shape):
    from sqmc_amd.host import HubbardKHost
    l_x, l_y = shape
    for t in (1.0, 0.7):
        h = HubbardKHost(l_x, l_y, 1, 1, t, 4.0)
        k, e = HK.k_table(l_x, l_y, t)
        assert h.k_vectors.tolist() == [list(x) for x in k]
        assert h.k_energies.tolist() == e              # the same doubles, not merely close
        assert (h.hf_up, h.hf_dn) == (1, 1)
    h = HubbardKHost(l_x, l_y, 2, 1)
    assert (h.hf_up, h.hf_dn) == (3, 1)                # the first nup / ndn orbitals of the order (k_hf_up, k_hf_dn)
    assert sorted(HK.HubbardKH(l_x, l_y, 1.0, 4.0).index) == sorted((2 * a, 2 * b) for a in range(l_x) for b in range(l_y))


@pytest.mark.parametrize("l_x,l_y,dim", [(3, 3, 324), (4, 3, 792)])
def test_spectrum_is_the_real_space_models(l_x, l_y, dim):
    """(nup, ndn) = (2, 1): every eigenvalue of the plane-wave matrix within 64 dim 2^-53 (lambda_max - lambda_min) of the
    real-space one (two symmetric eigensolves of a dim x dim matrix, each backward stable to a modest multiple of dim eps ||H||)"""
    t, U = 1.0, 4.0
    Hk, Hr = HK.HubbardKH(l_x, l_y, t, U), HK.real_space(l_x, l_y, t, U)
    dets = HK.all_determinants(l_x * l_y, 2, 1)
    assert len(dets) == dim
    wk = np.linalg.eigvalsh(HK.dense(Hk, dets, lambda u, d: HK.excitations_hubbardk(Hk, u, d)))
    wr = np.linalg.eigvalsh(HK.dense(Hr, dets, lambda u, d: PC.excitations_hubbard(Hr, u, d)))
    bound = 64.0 * dim * 2.0 ** -53 * (wr[-1] - wr[0])
    worst = float(np.max(np.abs(wk - wr)))
    print("%dx%d (2,1): %d determinants, worst eigenvalue difference %.3g, bound %.3g" % (l_x, l_y, dim, worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("l_x,l_y,nup,ndn", [(3, 3, 2, 2), (4, 3, 2, 1), (6, 1, 2, 2)])
def test_move_triples_are_the_row(l_x, l_y, nup, ndn):
    """for sampled parents the non-zero off-diagonal entries of the row of H (the element to EVERY determinant of the electron
    numbers) are the children of the move's triples, each child from exactly one triple, every |H| = U / N"""
    H = HK.HubbardKH(l_x, l_y, 1.0, 4.0)
    dets = HK.all_determinants(H.norb, nup, ndn)
    rng = random.Random(11)
    for par in [dets[0]] + rng.sample(dets, 5):
        nz = {c for c in dets if c != par and H.element(par[0], par[1], c[0], c[1])[0] != 0.0}
        kids = [tr[4] for tr in HK.triples_hubbardk(H, *par) if tr[4] is not None]
        assert len(kids) == len(set(kids))
        assert set(kids) == nz
        assert all(abs(H.element(par[0], par[1], c[0], c[1])[0]) == H.ubyn for c in kids)
        assert all(H.momentum(*c) == H.momentum(*par) for c in kids)
        assert len(HK.triples_hubbardk(H, *par)) == nup * ndn * (H.norb - nup)


def test_sector_partitions_the_space():
    H = HK.HubbardKH(3, 3, 1.0, 4.0)
    every = HK.all_determinants(9, 2, 2)
    parts = [HK.sector(H, 2, 2, (2 * a, 2 * b)) for a in range(3) for b in range(3)]
    assert sorted(d for p in parts for d in p) == every
    assert len(HK.sector(H, 2, 2, (0, 0))) == 144


def test_deck_parses_and_space_sym_is_refused():
    from sqmc_amd.walk_run import parse_walk_deck
    text = open(DECK).read()
    d = parse_walk_deck(text)
    assert d["hamiltonian_type"] == "hubbardk" and (d["l_x"], d["l_y"], d["nup"], d["ndn"]) == (4, 3, 2, 2)
    assert d["pbc"] is True and d["space_sym"] is False and (d["t"], d["U"]) == (1.0, 4.0) and d["proposal_method"] == "uniform2"
    lines = text.splitlines()
    k = [i for i, l in enumerate(lines) if l.rstrip().endswith("space_sym")][0]
    lines[k] = "t" + lines[k][1:]
    with pytest.raises(SystemExit) as ei:
        parse_walk_deck("\n".join(lines))
    assert "space_sym" in str(ei.value)
