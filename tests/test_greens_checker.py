"""tests/greens_checker.py against explicit Jordan-Wigner matrices on a whole Fock space and against the 1-RDM sum rule, and the host-side
pieces of the Green's function stage that need no GPU: the frequency grid, the density of states, the three files, the deck group."""
import itertools
import math
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import greens_checker as GC       # noqa: E402
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402

DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
NORB = 4


class ModelH(PC.Hamiltonian):
    """dense seeded integrals on NORB orbitals: h_pq symmetric, (pq|rs) with the eightfold symmetry, both diagonal in spin"""

    def __init__(self, seed):
        rng = random.Random(seed)
        self.norb, self.const = NORB, rng.uniform(-1.0, 1.0)
        self.h1 = {(p, q): rng.uniform(-1.0, 1.0) for p in range(NORB) for q in range(p + 1)}
        self.h2 = {}
        for p, q, r, s in itertools.product(range(NORB), repeat=4):
            self.h2.setdefault(PC._eri_key(p, q, r, s), rng.uniform(-0.5, 0.5))

    def t(self, P, Q):
        n = self.norb
        return self.h1[(max(P % n, Q % n), min(P % n, Q % n))] if P // n == Q // n else 0.0

    def v(self, P, Q, R, S):
        n = self.norb
        return self.h2[PC._eri_key(P % n, Q % n, R % n, S % n)] if P // n == Q // n and R // n == S // n else 0.0


def _jordan_wigner(H):
    """a_P as dense matrices on the 2^(2 norb) states |I>, I = up | dn << norb, a_P |I> = (-1)^(bits of I below P) |I - P>; and H"""
    m = 2 * H.norb
    dim = 1 << m
    a = []
    for P in range(m):
        mat = np.zeros((dim, dim))
        for I in range(dim):
            if I >> P & 1:
                mat[I ^ (1 << P), I] = -1.0 if bin(I & ((1 << P) - 1)).count("1") & 1 else 1.0
        a.append(mat)
    ham = H.const * np.eye(dim)
    for P in range(m):
        for Q in range(m):
            if H.t(P, Q) != 0.0:
                ham += H.t(P, Q) * (a[P].T @ a[Q])
    pairs = [(x, y) for x in range(m) for y in range(m)]
    B = np.array([a[y] @ a[x] for x, y in pairs]).reshape(len(pairs), -1)           # B[(Q, S)] = a_S a_Q
    V = np.array([[H.v(P, Q, R, S) for (Q, S) in pairs] for (P, R) in pairs])       # a+_P a+_R = (a_R a_P)^T = B[(P, R)]^T
    Cm = (V @ B).reshape(len(pairs), dim, dim)
    B = B.reshape(len(pairs), dim, dim)
    for k in range(len(pairs)):
        ham += 0.5 * (B[k].T @ Cm[k])
    return a, ham


_JW = {}


def _model():
    if not _JW:
        H = ModelH(3)
        _JW["H"] = H
        _JW["a"], _JW["ham"] = _jordan_wigner(H)
        assert np.max(np.abs(_JW["ham"] - _JW["ham"].T)) < 1e-12
    return _JW["H"], _JW["a"], _JW["ham"]


def _sector(nup, ndn):
    strings = lambda k: [sum(1 << o for o in c) for c in itertools.combinations(range(NORB), k)]
    return [(u, d) for u in strings(nup) for d in strings(ndn)]


@pytest.mark.parametrize("nup,ndn", [(1, 1), (2, 1), (1, 2)])
def test_checker_against_jordan_wigner(nup, ndn):
    H, a, ham = _model()
    dim, D = ham.shape[0], np.diag(ham)
    rng = random.Random(10 * nup + ndn)
    dets = _sector(nup, ndn)
    rng.shuffle(dets)
    dets = dets[:max(3, (2 * len(dets)) // 3)]                 # part of the sector: some k are not in the list
    c = [rng.uniform(-1.0, 1.0) for _ in dets]
    psi = np.zeros(dim)
    for (u, d), x in zip(dets, c):
        psi[H.state(u, d)] = x
    e0 = -0.7
    chk = GC.Greens(H, dets, c, e0, NORB)
    for (u, d) in _sector(nup + 1, ndn)[:4]:                   # the checker's H_mm is the diagonal of the dense H in the N+1 sector
        assert abs(chk.diagonal(u, d)[0] - D[H.state(u, d)]) < 1e-12
    freqs = GC.outside(chk.all_poles(), 0.8) + GC.in_gaps(chk.all_poles(), 1, 0.0)
    n_off = 0
    for w in freqs:
        rp, rm = 1.0 / (w - (D - e0)), 1.0 / (w - (e0 - D))
        for p in range(NORB):
            for q in range(NORB):
                for part, res in ((GC.NP1, rp), (GC.NM1, rm)):
                    sg = un = 0.0
                    for sigma in (0, 1):
                        ap, aq = a[p + sigma * NORB], a[q + sigma * NORB]
                        left, right = (ap.T, aq.T) if part == GC.NP1 else (ap, aq)       # <psi| a_p R a+_q |psi>  /  <psi| a+_p R a_q |psi>
                        sg += (left @ psi) @ (res * (right @ psi))
                        un += (np.abs(left) @ psi) @ (res * (np.abs(right) @ psi))
                    e = chk.entry(part, p, q, w)
                    assert abs(e.signed - sg) < 1e-12 and abs(e.unsigned - un) < 1e-12, (part, p, q, w)
                    if p == q:
                        assert e.signed == e.unsigned
                    elif e.n and abs(sg - un) > 1e-6:
                        n_off += 1
    assert n_off > 0                                           # the two modes do differ somewhere off the diagonal


@pytest.mark.parametrize("nup,ndn", [(2, 1), (2, 2)])
def test_sum_rule_against_the_one_rdm(nup, ndn):
    """all residues summed, signed mode: R_np1(p, q) = <a_p a+_q> = 2 delta_pq sum c^2 - <a+_q a_p>, R_nm1(p, q) = <a+_p a_q>; rdm_checker's
    M[p][r] = <a+_r a_p>"""
    H, _, _ = _model()
    rng = random.Random(nup + 5 * ndn)
    dets = _sector(nup, ndn)
    rng.shuffle(dets)
    dets = dets[:(3 * len(dets)) // 4]
    c = [rng.uniform(-1.0, 1.0) for _ in dets]
    chk = GC.Greens(H, dets, c, -0.3, NORB)
    rdm = RC.one_rdm(dets, c, NORB)
    norm = math.fsum(x * x for x in c)
    rp, rm = chk.residues(GC.NP1), chk.residues(GC.NM1)
    for p in range(NORB):
        for q in range(NORB):
            assert abs(rm.get((p, q), (0.0,))[0] - rdm.value(q, p)) < 1e-13
            assert abs(rp.get((p, q), (0.0,))[0] - ((2.0 * norm if p == q else 0.0) - rdm.value(p, q))) < 1e-13


def test_frequency_choosers():
    poles = [-3.0, -2.9, -1.0, 0.5, 0.55, 2.0]
    assert GC.outside(poles, 0.5) == [-3.5, 2.5]
    assert GC.in_gaps(poles, 2) == [-1.95, -0.25]
    with pytest.raises(AssertionError):
        GC.in_gaps(poles, 5)                                   # the fifth gap is 0.05 wide
    w_min, w_max = GC.uniform(poles, 5)
    grid = [w_min + (w_max - w_min) * i / 4.0 for i in range(5)]
    assert all(min(abs(w - x) for x in poles) >= GC.D_MIN for w in grid) and w_min < -3.0 and w_max > 2.0


# ---------------------------------------------------------------------------------------------- host side
def test_grid_and_density_of_states():
    from sqmc_amd import host as H
    w = H.greens_grid(5, -1.0, 2.0)
    assert w.tolist() == [-1.0 + 3.0 * i / 4.0 for i in range(5)] and w[0] == -1.0 and w[-1] == 2.0
    assert H.greens_grid(2, 0.5, 0.25).tolist() == [0.5, 0.25]
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            H.greens_grid(bad, 0.0, 1.0)
    rng = np.random.default_rng(4)
    gp, gm = rng.normal(size=(3, 5, 5)), rng.normal(size=(3, 5, 5))
    rho = H.density_of_states(gp, gm)
    assert rho.shape == (3, 3)
    for i in range(3):
        a = b = 0.0
        for p in range(5):
            a += gp[i, p, p]; b += gm[i, p, p]
        assert rho[i, 0] == a and rho[i, 1] == b and rho[i, 2] == a + b


def test_files_round_trip(tmp_path):
    from sqmc_amd import host as H
    rng = np.random.default_rng(7)
    n_w, n = 4, 6
    w = H.greens_grid(n_w, -2.0, 1.0)
    gp, gm = rng.normal(size=(n_w, n, n)), rng.normal(size=(n_w, n, n)) * 1e-3
    gp[1, 2, 3], gp[1, 3, 2], gp[2, 0, 0], gm[0, 5, 5] = 0.99e-8, -1.01e-8, 1e-8, -2e-8      # around the cut: abs > 1e-8 is written
    paths = H.write_greens_function(str(tmp_path), w, gp, gm)
    assert sorted(os.path.basename(x) for x in paths.values()) == ["G0_N+1", "G0_N-1", "rho"]
    for name, g in (("G0_N+1", gp), ("G0_N-1", gm)):
        header, rec = H.read_greens_function(paths[name])
        assert header == " w,p,q,G0_{N%s1}(w,p,q)" % name[-2]
        want = [(w[i], p + 1, q + 1, g[i, p, q]) for i in range(n_w) for q in range(n) for p in range(n) if abs(g[i, p, q]) > 1e-8]
        assert rec == want                                     # 17 significant digits: every double comes back; order i_w, then q, then p
    _, rec = H.read_greens_function(paths["G0_N+1"])
    keys = {(r[0], r[1], r[2]) for r in rec}
    assert (w[1], 3, 4) not in keys and (w[1], 4, 3) in keys and (w[2], 1, 1) not in keys
    assert (w[0], 6, 6) in {(r[0], r[1], r[2]) for r in H.read_greens_function(paths["G0_N-1"])[1]}
    line = open(paths["G0_N+1"]).readlines()[1]
    import re
    real = r"[ -]\d\.\d{16}E[+-]\d{3}"                          # es24.16e3
    assert re.fullmatch(real + r"[ \d]{5}[ \d]{5}" + real + "\n", line), line
    header, rho = H.read_greens_function(paths["rho"])
    assert header == " Density of states: w, rho_{N+1}(w),rho_{N-1}(w),rho_tot(w)"
    assert np.array_equal(rho[:, 0], w) and np.array_equal(rho[:, 1:], H.density_of_states(gp, gm))
    assert np.array_equal(rho[:, 3], rho[:, 1] + rho[:, 2])


@pytest.mark.parametrize("present", ["G0_N+1", "G0_N-1", "rho"])
def test_no_file_is_overwritten(tmp_path, present):
    from sqmc_amd import host as H
    (tmp_path / present).write_text("mine\n")
    g = np.ones((2, 3, 3))
    with pytest.raises(FileExistsError):
        H.write_greens_function(str(tmp_path), [0.0, 1.0], g, g)
    assert sorted(os.listdir(tmp_path)) == [present] and (tmp_path / present).read_text() == "mine\n"      # checked before any file is made


def test_deck_group():
    from sqmc_amd import run as R
    text = open(DECK).read()
    off = R.parse_hci_deck(text)
    assert off["get_greens_function"] is False and off["n_w"] == 20 and off["w_min"] is None and off["w_max"] is None
    d = R.parse_hci_deck(text + "&greens_function get_greens_function=t n_w=7 w_min=-1.5d0 w_max=2.25 /\n")
    assert d["get_greens_function"] is True and d["n_w"] == 7 and d["w_min"] == -1.5 and d["w_max"] == 2.25
    assert d["get_natorbs"] is False and d["n_states"] == off["n_states"] and d["eps_var_sched"] == off["eps_var_sched"]
    d = R.parse_hci_deck(text + "&greens_function\n get_greens_function = .true.\n w_min = -1.d0, w_max = 1.d-1\n/\n")
    assert d["get_greens_function"] and d["n_w"] == 20 and d["w_min"] == -1.0 and d["w_max"] == 0.1
    d = R.parse_hci_deck(text + "&greens_function get_greens_function=f n_w=3 /\n")
    assert d["get_greens_function"] is False and d["n_w"] == 3


def test_deck_stops_before_any_work(tmp_path, monkeypatch):
    """n_w < 2, a missing w_min / w_max, an existing file, and a HEG deck: each stops with a message before a device is touched"""
    from sqmc_amd import run as R
    monkeypatch.chdir(tmp_path)
    text = open(DECK).read()
    for group, word in (("get_greens_function=t n_w=1 w_min=0.0 w_max=1.0", "n_w"), ("get_greens_function=t n_w=4 w_max=1.0", "w_min"),
                        ("get_greens_function=t n_w=4 w_min=1.0", "w_min and w_max")):
        with pytest.raises(SystemExit) as e:
            R.run_hci(R.parse_hci_deck(text + "&greens_function %s /\n" % group), os.path.join(tmp_path, "no_such_FCIDUMP"))
        assert word in str(e.value)
    (tmp_path / "rho").write_text("mine\n")
    with pytest.raises(FileExistsError):
        R.run_hci(R.parse_hci_deck(text + "&greens_function get_greens_function=t n_w=4 w_min=0.0 w_max=1.0 /\n"), os.path.join(tmp_path, "no_such_FCIDUMP"))
    heg = R.parse_hci_deck(open(os.path.join(ROOT, "tests", "golden", "heg_e2e_i_det")).read() + "&greens_function get_greens_function=t w_min=0.0 w_max=1.0 /\n")
    assert heg["get_greens_function"]
    with pytest.raises(SystemExit) as e:
        R.run_hci(heg)
    assert "chem only" in str(e.value)
