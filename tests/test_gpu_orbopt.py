"""sqmc_gpu_orbital_gradient on the MI355X against tests/orbopt_checker.py: every entry of the Fock matrix, the gradient and the diagonal
Hessian at the edge sizes and on both sides of the kernels' seams within the derived rounding bounds, the exact properties with ==,
the C2 fixture end to end through the rotation door, a complete space, the orbital step, the deck runner, the refusals and the scratch."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import orbopt_checker as OC       # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
OK, BAD_ARG, ERR_HIP, UNSUPPORTED = 0, -1, -2, -3
V = C.c_void_p
# 2 (one pair), 3 and 5 (K = norb^3 no multiple of the chunk of 16 triples); 20 | 21: one chunk per block | two (more than 512
# chunks); 32 | 33: 2 x 2 | 4 x 4 register tiles.  test_the_sizes_straddle_every_seam holds the list to the kernels' own constants.
SEAM_SIZES = [20, 21, 32, 33]
EDGE_SIZES = [2, 3, 5] + SEAM_SIZES
NAMES = ("fock", "gradient", "hdiag")


@pytest.fixture(scope="module")
def dev():
    import sqmc_amd
    sqmc_amd.set_device(0)
    return sqmc_amd


# ------------------------------------------------------------------------------------------------------------------ synthetic systems
_SYS, _CTX = {}, []


def _pack(host, h, e, core):
    """dense integrals over the context's orbitals into the host's packed table (this test's own addressing through combine_2)"""
    n, n1, c2 = host.norb, host.norb + 1, host.combine_2
    pr = c2[1:n1, 1:n1].astype(np.int64)
    packed = np.zeros_like(host.integrals)
    hi, lo = np.maximum(pr[:, :, None, None], pr[None, None, :, :]), np.minimum(pr[:, :, None, None], pr[None, None, :, :])
    packed[(hi * (hi - 1)) // 2 + lo] = e
    A = int(c2[n1, n1])
    packed[A * (A - 1) // 2 + pr] = h
    packed[A * (A - 1) // 2 + A] = core
    return packed


class _System:
    pass


def _system(dev, tmp_path_factory, norb, seed=None, symmetric_g=True, nelec=2, nup=1):
    """seeded random dense integrals, a symmetric D and G symmetrised to G[p,q,r,s] = G[r,s,p,q] = G[q,p,s,r] (or not), and a c1 chem
    context that holds the integrals; kept for the module"""
    from sqmc_amd import host as H
    seed = 7000 + norb if seed is None else seed
    key = (norb, seed, symmetric_g, nelec, nup)
    if key not in _SYS:
        s = _System()
        s.norb = norb
        s.h, s.e, s.D, s.G = OC.random_system(norb, seed, symmetric_g)
        path = str(tmp_path_factory.mktemp("orbopt%d" % norb) / "FCIDUMP")
        with open(path, "w") as f:          # a placeholder with the right header: the integrals come from with_integrals
            f.write(" &FCI NORB=%d,NELEC=%d,MS2=0,\n  ORBSYM=%s,\n  ISYM=1,\n &END\n" % (norb, nelec, ",".join(["1"] * norb)))
            f.write("".join("%.17e %d %d 0 0\n" % (0.5 + p, p + 1, p + 1) for p in range(norb)) + "%.17e 0 0 0 0\n" % -1.5)
        base = H.ChemHost(path, nelec, nup, "c1")
        s.host = base.with_integrals(_pack(base, s.h, s.e, -1.5))
        s.g = s.host.gpu()
        _CTX.append(s.g)
        _SYS[key] = s
    return _SYS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for g in _CTX:
        g.close()
    _CTX.clear(); _SYS.clear()


def _no_negative_zero(out):
    for k, a in out.items():
        assert not np.signbit(a[a == 0.0]).any(), k


def _exact_properties(out):
    g, hd = out["gradient"], out["hdiag"]
    assert np.array_equal(g, -g.T) and np.all(np.diag(g) == 0.0) and np.all(np.diag(hd) == 0.0)
    _no_negative_zero(out)


# ----------------------------------------------------------------------------------------------------------------------------- tests
def test_the_sizes_straddle_every_seam(dev):
    """the sizes at which the Fock GEMM changes its register tile or its chunks per block, from the library's own plan"""
    L = dev.load_library()
    L.sqmc_gpu_debug_orbopt_plan.argtypes = [C.c_int32, V]
    plans = {}
    for n in range(1, 65):
        out = (C.c_int64 * 4)()
        assert L.sqmc_gpu_debug_orbopt_plan(n, out) == OK
        plans[n] = tuple(out)                          # (register tile, triples per chunk, chunks per block, blocks)
    assert plans[2][1] == 16 and plans[2][3] == 1 and plans[64][3] == 512
    tile = [n for n in range(2, 65) if plans[n][0] != plans[n - 1][0]]
    split = [n for n in range(2, 65) if plans[n - 1][2] == 1 and plans[n][2] > 1]
    assert tile == [33] and split == [21]
    for n in tile + split:
        assert n in SEAM_SIZES and n - 1 in SEAM_SIZES
    assert any(n ** 3 % plans[n][1] for n in EDGE_SIZES) and any(plans[n][3] > 1 for n in EDGE_SIZES)


@pytest.mark.parametrize("norb", EDGE_SIZES)
def test_edge_sizes(dev, tmp_path_factory, norb):
    """every entry of the three outputs against the checker: fock against the literal sum in longdouble, gradient and hdiag against
    the Fourier derivatives of the energy"""
    s = _system(dev, tmp_path_factory, norb)
    out = s.g.orbital_gradient(s.D, s.G)
    assert sorted(out) == sorted(NAMES) and all(a.shape == (norb, norb) and a.dtype == np.float64 for a in out.values())
    _exact_properties(out)
    fabs = OC.fock_abs(s.h, s.e, s.D, s.G)
    fb = OC.fock_bound(norb, fabs)
    df = np.abs(out["fock"] - np.asarray(OC.fock_literal(s.h, s.e, s.D, s.G), float))
    d1, d2 = OC.all_pair_derivatives(s.h, s.e, s.D, s.G)
    pairs = [(p, q) for p in range(norb) for q in range(norb) if p != q]
    habs = OC.hdiag_abs(s.h, s.e, s.D, s.G, pairs, fabs)
    wg = wh = 0.0
    for p, q in pairs:
        wg = max(wg, abs(out["gradient"][p, q] - float(d1[p, q])) / OC.gradient_bound(norb, fabs, p, q))
        wh = max(wh, abs(out["hdiag"][p, q] - float(d2[p, q])) / OC.hdiag_bound(norb, habs[(p, q)]))
    print("norb = %d: worst |delta| / bound: fock %.4f, gradient %.4f, hdiag %.4f" % (norb, float(np.max(df / fb)), wg, wh))
    assert np.all(df <= fb) and wg <= 1.0 and wh <= 1.0


def test_64_orbitals_on_a_sample(dev, tmp_path_factory):
    norb = 64
    s = _system(dev, tmp_path_factory, norb)
    out = s.g.orbital_gradient(s.D, s.G)
    _exact_properties(out)
    rng = np.random.default_rng(64)
    fabs = OC.fock_abs(s.h, s.e, s.D, s.G)
    entries = [(0, 0), (63, 63), (0, 63), (63, 0), (31, 32)] + [tuple(int(x) for x in rng.integers(0, norb, 2)) for _ in range(24)]
    worst = 0.0
    for (a, P), want in OC.fock_entries(s.h, s.e, s.D, s.G, entries).items():
        d, b = abs(out["fock"][a, P] - float(want)), OC.fock_bound(norb, fabs[a, P])
        assert d <= b, (a, P, d, b)
        worst = max(worst, d / b)
    pairs = [(0, 1), (63, 0), (31, 32), (62, 63)] + [tuple(int(x) for x in rng.choice(norb, 2, replace=False)) for _ in range(4)]
    habs = OC.hdiag_abs(s.h, s.e, s.D, s.G, pairs, fabs)
    wg = wh = 0.0
    for (p, q), (d1, d2) in OC.derivatives(s.h, s.e, s.D, s.G, pairs).items():
        wg = max(wg, abs(out["gradient"][p, q] - float(d1)) / OC.gradient_bound(norb, fabs, p, q))
        wh = max(wh, abs(out["hdiag"][p, q] - float(d2)) / OC.hdiag_bound(norb, habs[(p, q)]))
    print("norb = 64: worst |delta| / bound: fock %.4f, gradient %.4f, hdiag %.4f" % (worst, wg, wh))
    assert wg <= 1.0 and wh <= 1.0


@pytest.mark.parametrize("norb", [5, 21, 33])
def test_same_bits_again_alone_and_from_a_second_context(dev, tmp_path_factory, norb):
    s = _system(dev, tmp_path_factory, norb)
    first = s.g.orbital_gradient(s.D, s.G)
    again = s.g.orbital_gradient(s.D, s.G)
    g2 = s.host.gpu()
    _CTX.append(g2)
    other = g2.orbital_gradient(s.D, s.G)
    for k in NAMES:
        assert first[k].tobytes() == again[k].tobytes() == other[k].tobytes(), k
        alone = s.g.orbital_gradient(s.D, s.G, k)
        assert list(alone) == [k] and alone[k].tobytes() == first[k].tobytes(), k
    two = s.g.orbital_gradient(s.D, s.G, ("gradient", "hdiag"))
    assert sorted(two) == ["gradient", "hdiag"] and all(two[k].tobytes() == first[k].tobytes() for k in two)


@pytest.mark.parametrize("norb", [3, 33])
def test_zero_matrices_give_zero_outputs(dev, tmp_path_factory, norb):
    s = _system(dev, tmp_path_factory, norb)
    out = s.g.orbital_gradient(np.zeros((norb, norb)), np.zeros((norb,) * 4))
    for k in NAMES:
        assert not out[k].any() and not np.signbit(out[k]).any(), k


@pytest.mark.parametrize("norb", [5, 21])
def test_unsymmetrised_matrices_take_the_literal_formula(dev, tmp_path_factory, norb):
    """G as drawn, D not symmetric: fock is the formula as written, and the exact properties do not depend on the symmetries"""
    s = _system(dev, tmp_path_factory, norb, seed=7100 + norb, symmetric_g=False)
    D = s.D + np.triu(np.random.default_rng(5).uniform(-1, 1, (norb, norb)), 1)
    assert not np.array_equal(D, D.T) and not np.array_equal(s.G, s.G.transpose(2, 3, 0, 1))
    out = s.g.orbital_gradient(D, s.G)
    _exact_properties(out)
    fabs = OC.fock_abs(s.h, s.e, D, s.G)
    df = np.abs(out["fock"] - np.asarray(OC.fock_literal(s.h, s.e, D, s.G), float))
    assert np.all(df <= OC.fock_bound(norb, fabs))
    assert np.abs(out["fock"] - np.asarray(OC.fock_literal(s.h, s.e, D.T, s.G.transpose(2, 3, 0, 1)), float)).max() > 1e-3      # the other reading differs


def test_the_host_yardstick_agrees(dev, tmp_path_factory):
    from sqmc_amd import host as H
    norb = 21
    s = _system(dev, tmp_path_factory, norb)
    h, e, _ = H.dense_integrals(s.host)
    assert np.array_equal(h, s.h) and np.array_equal(e, s.e)
    out, ref = s.g.orbital_gradient(s.D, s.G), H.orbital_gradient_host(s.host, s.D, s.G)
    fabs = OC.fock_abs(s.h, s.e, s.D, s.G)
    pairs = [(p, q) for p in range(norb) for q in range(norb) if p != q]
    habs = OC.hdiag_abs(s.h, s.e, s.D, s.G, pairs, fabs)
    assert np.all(np.abs(out["fock"] - ref["fock"]) <= 2 * OC.fock_bound(norb, fabs))
    for p, q in pairs:
        assert abs(out["gradient"][p, q] - ref["gradient"][p, q]) <= 2 * OC.gradient_bound(norb, fabs, p, q)
        assert abs(out["hdiag"][p, q] - ref["hdiag"][p, q]) <= 2 * OC.hdiag_bound(norb, habs[(p, q)])


# ----------------------------------------------------------------------------------------------------------------------- C2 fixture
@pytest.fixture(scope="module")
def c2(dev):
    """C2 cc-pVDZ, 8 electrons in 26 orbitals, d2h, no time_sym: two states after one iteration at eps_var 5e-3 (a few hundred
    determinants of the 10^8 of the space), the density matrices of state 1 and a context"""
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", hf_symmetry=1)
    g = h.gpu()
    _CTX.append(g)
    g.set_hb_tables(*h.hb_tables(g))
    up, dn, w, e, hist = H.hci_variational(h, g, 5e-3, n_states=2, max_iters=1)
    assert 50 <= len(up) <= 3000, hist
    w = np.asarray(w, float).reshape(len(up), -1)
    s = _System()
    s.h, s.g, s.up, s.dn, s.w, s.e = h, g, up, dn, w, e
    s.D = H.hci_one_rdm(h, up, dn, w[:, 0])
    s.G = H.spin_free_two_rdm(H.hci_two_rdm(h, up, dn, w[:, 0]))
    s.sym = np.asarray(h.orbsym[1:h.norb + 1])
    return s


def test_c2_gradient_is_zero_between_irreps_and_is_the_derivative_of_the_rotated_energy(c2):
    from sqmc_amd import host as H
    h, g, n = c2.h, c2.g, c2.h.norb
    out = g.orbital_gradient(c2.D, c2.G)
    _exact_properties(out)
    diff = c2.sym[:, None] != c2.sym[None, :]
    assert diff.any() and np.all(out["gradient"][diff] == 0.0) and np.all(out["fock"][diff] == 0.0)
    same = [(p, q) for p in range(n) for q in range(p + 1, n) if c2.sym[p] == c2.sym[q]]
    big = sorted(same, key=lambda pq: -abs(out["gradient"][pq]))
    pairs = [big[0], big[len(big) // 2], (0, next(q for q in range(1, n) if c2.sym[q] == c2.sym[0]))]
    dh, de, core = OC.read_fcidump_dense(FCIDUMP, [int(h.orb_order[i]) for i in range(1, n + 1)])
    n2 = float(np.trace(c2.D)) / 8
    for p, q in pairs:
        samples, delta = [], 0.0
        for j in range(OC.ANGLES):
            U = np.asarray(OC.plane_rotation(n, p, q, 2 * OC.PI * j / OC.ANGLES), float)
            samples.append(H.rdm_energy(h.with_integrals(g.rotate_integrals(U)), c2.D, c2.G))
            delta = max(delta, OC.energy_bound(dh, de, c2.D, c2.G, U, core * n2))
        d1, _ = OC.fourier_derivatives(samples)
        print("C2 pair (%d, %d): g = %.10e, Fourier derivative of 9 rotated energies = %.10e, |delta g| = %.2e, 20 delta = %.2e"
              % (p, q, out["gradient"][p, q], float(d1), abs(out["gradient"][p, q] - float(d1)), 20 * delta))
        assert abs(out["gradient"][p, q] - float(d1)) <= 20 * delta
    assert abs(out["gradient"][pairs[0]]) > 1e3 * 20 * delta        # a truncated space: the largest entry stands far above the bound


def test_c2_optimize_orbitals_step(c2):
    from sqmc_amd import host as H
    h, n = c2.h, c2.h.norb
    r = H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, 0])
    U = r["rotation"]
    assert r["energy_after"] < r["energy_before"] and 0.0 < r["scale"] <= 1.0 and 0.0 < r["max_kappa"] <= H.ORBOPT_MAX_STEP
    assert abs(r["energy_before"] - c2.e[0]) < 1e-6
    assert np.max(np.abs(U.T @ U - np.eye(n))) <= n * 2.0 ** -50
    assert np.all(U[c2.sym[:, None] != c2.sym[None, :]] == 0.0)
    assert r["max_gradient"] == np.max(np.abs(r["gradient"])) and r["integrals"].shape == h.integrals.shape
    assert H.rdm_energy(h.with_integrals(r["integrals"]), c2.D, c2.G) == r["energy_after"]
    h2 = h.with_integrals(r["integrals"])
    g2 = h2.gpu()
    _CTX.append(g2)
    g2.set_hb_tables(*h2.hb_tables(g2))
    up, dn, w, e, hist = H.hci_variational(h2, g2, 5e-3, max_iters=1)
    assert len(up) > 1 and np.isfinite(e[0])
    print("C2: E(D, G) %.9f -> %.9f at scale %g, max|g| %.3e; HCI in the new orbitals: %d determinants, E_var %.9f (was %d, %.9f)"
          % (r["energy_before"], r["energy_after"], r["scale"], r["max_gradient"], len(up), e[0], len(c2.up), c2.e[0]))


def test_c2_state_average_is_the_door_on_the_averaged_matrices(c2):
    from sqmc_amd import host as H
    h = c2.h
    r = H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, :2], max_halvings=0)
    d = [H.hci_two_rdm(h, c2.up, c2.dn, c2.w[:, i]) for i in (0, 1)]
    D = (H.hci_one_rdm(h, c2.up, c2.dn, c2.w[:, 0]) + H.hci_one_rdm(h, c2.up, c2.dn, c2.w[:, 1])) / 2
    G = H.spin_free_two_rdm({b: (d[0][b] + d[1][b]) / 2 for b in d[0]})
    assert np.array_equal(r["one_rdm"], D) and np.array_equal(r["two_rdm_sf"], G)
    out = c2.g.orbital_gradient(D, G)
    assert r["gradient"].tobytes() == out["gradient"].tobytes() and r["hdiag"].tobytes() == out["hdiag"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- complete space
def test_gradient_vanishes_for_the_exact_ground_state_of_a_complete_space(dev, tmp_path_factory):
    """3 electrons in 4 orbitals, all 24 determinants, coefficients from eigh of the checker's H; the density matrices from the
    library's own doors.  1e-9 max|F| is a generous margin over eigh's n 2^-53 ||H||, not a measurement."""
    from sqmc_amd import host as H
    norb = 4
    s = _system(dev, tmp_path_factory, norb, nelec=3, nup=2)
    dets = OC.complete_space(norb, 2, 1)
    Hm = OC.hamiltonian_matrix(OC.dense_hamiltonian(s.h, s.e, -1.5), dets)
    c = np.linalg.eigh((Hm + Hm.T) / 2)[1][:, 0]
    up, dn = np.array([a for a, _ in dets], np.uint64), np.array([b for _, b in dets], np.uint64)

    def grad(keep):
        D = s.g.one_rdm(up[keep], dn[keep], c[keep], None)
        G = H.spin_free_two_rdm(s.g.two_rdm(up[keep], dn[keep], c[keep]))
        out = s.g.orbital_gradient(D, G)
        return float(np.max(np.abs(out["gradient"]))), float(np.max(np.abs(out["fock"])))
    g_full, f_full = grad(np.arange(len(dets)))
    g_half, _ = grad(np.argsort(-np.abs(c), kind="stable")[:len(dets) // 2])
    print("complete space: max|g| = %.3e, max|F| = %.3e; truncated to half: max|g| = %.3e" % (g_full, f_full, g_half))
    assert g_full < 1e-9 * f_full and g_half > 1e-3 * f_full


# ----------------------------------------------------------------------------------------------------------------------------- deck
def _deck_text():
    t = open(DECK).read().replace("1e-3  1e-7", "5e-3  1e-5").replace("eps_var_sched=2*2e-3", "eps_var_sched=2*1e-2")
    assert "5e-3  1e-5" in t and "2*1e-2" in t
    return t


def test_deck_with_optimize_orbitals(dev, tmp_path):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    buf, path = io.StringIO(), str(tmp_path / "FCIDUMP_opt")
    res = R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=buf, optimize_orbitals=path)
    lines = buf.getvalue().splitlines()
    first = "Orbital optimisation: one diagonal-Newton step from the 1-RDM and the 2-RDM of the variational wavefunction"
    last = "Rotated integrals written to " + path
    i0, i1 = lines.index(first), lines.index(last)
    assert i1 == i0 + 5 and lines[i0 - 1] == ""
    assert lines[i0 + 1].startswith(" Energy from the density matrices =") and "Variational energy =" in lines[i0 + 1]
    assert lines[i0 + 2].startswith(" max|g| =") and "||g||_2 =" in lines[i0 + 2]
    assert lines[i0 + 3].startswith(" max|kappa| =") and "backtracking scale =" in lines[i0 + 3]
    assert lines[i0 + 4].startswith(" Fixed-coefficient energy after the step =")
    o = res["optimize_orbitals"]
    assert o["energy_after"] < o["energy_before"] and o["scale"] > 0.0
    assert lines.index("State   1:") > i1                       # the PT stage follows
    # the file reads back to the rotated integrals at its 13 digits
    deck = R.parse_hci_deck(_deck_text())
    h = H.ChemHost(FCIDUMP, deck["nelec"], deck["nup"], deck["point_group"], time_sym=deck["time_sym"], z=deck["z"], hf_symmetry=deck["hf_symmetry"])
    n, n1 = h.norb, h.norb + 1
    norb, orbsym, vals, idx = H.read_fcidump(path)
    assert norb == n and list(orbsym) == [int(x) for x in h.orbsym_file[1:n1]]
    inv = np.zeros(n1 + 1, np.int64); inv[np.asarray(h.orb_order[1:n1], np.int64)] = np.arange(1, n1); inv[0] = n1
    ctx = inv[idx]
    want = o["integrals"][H.ChemHost._index(h.combine_2, ctx[:, 0], ctx[:, 1], ctx[:, 2], ctx[:, 3])]
    assert len(vals) > n and np.all(np.abs(vals - want) <= 5.01e-13 * np.abs(want))
    tri = [(p, q) for p in range(1, n1) for q in range(1, p + 1)]
    one = o["integrals"][H.ChemHost._index(h.combine_2, np.array([p for p, _ in tri]), np.array([q for _, q in tri]), np.full(len(tri), n1), np.full(len(tri), n1))]
    assert int(np.sum((idx[:, 2] == 0) & (idx[:, 0] != 0))) == int(np.sum(np.abs(one) > 1e-8))
    # new files only
    with pytest.raises(FileExistsError):
        R.run_optimize_orbitals(None, None, None, None, None, None, path)
    # the same deck without the flag: exactly the lines of before (all but the last, which reports wall-clock times)
    buf2 = io.StringIO()
    res2 = R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=buf2)
    plain = buf2.getvalue().splitlines()
    assert "Orbital optimisation" not in buf2.getvalue() and "optimize_orbitals" not in res2
    stage = set(range(i0 - 1, i1 + 1))
    rest = [l for k, l in enumerate(lines) if k not in stage]
    assert rest[:-1] == plain[:-1] and rest[-1].startswith("sqmc_amd: variational stage") and plain[-1].startswith("sqmc_amd: variational stage")
    assert res2["states"] == res["states"]


def test_deck_refusals(dev, tmp_path):
    from sqmc_amd import run as R
    path = str(tmp_path / "never")
    for change in (dict(hamiltonian_type="heg"), dict(get_natorbs=True), dict(n_energy_batch=2)):
        deck = R.parse_hci_deck(_deck_text())
        deck.update(change)
        with pytest.raises(SystemExit) as e:
            R.run_hci(deck, FCIDUMP, out=io.StringIO(), optimize_orbitals=path)
        assert "--optimize-orbitals" in str(e.value) and not os.path.exists(path)


# ------------------------------------------------------------------------------------------------------------- refusals and scratch
def _raw(L, ctx, D, G, outs):
    L.sqmc_gpu_orbital_gradient.argtypes = [V] * 6
    ptr = lambda a: None if a is None else a.ctypes.data_as(V)
    return L.sqmc_gpu_orbital_gradient(ctx, ptr(D), ptr(G), *[ptr(a) for a in outs])


def test_refusals_leave_the_outputs_untouched(dev, tmp_path_factory):
    from sqmc_amd import host as H
    norb = 5
    s = _system(dev, tmp_path_factory, norb)
    L = s.g.L
    D, G = np.ascontiguousarray(s.D.reshape(-1, order="F")), np.ascontiguousarray(s.G.reshape(-1, order="F"))
    outs = [np.full(norb * norb, 7.25) for _ in range(3)]
    untouched = lambda: all(bool(np.all(a == 7.25)) for a in outs)
    assert _raw(L, None, D, G, outs) == BAD_ARG and untouched()
    assert _raw(L, s.g.h, None, G, outs) == BAD_ARG and _raw(L, s.g.h, D, None, outs) == BAD_ARG and untouched()
    assert _raw(L, s.g.h, D, G, [None, None, None]) == BAD_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            d, gg = D.copy(), G.copy()
            (d, gg)[which][-1] = bad
            assert _raw(L, s.g.h, d, gg, outs) == BAD_ARG and untouched()
    with pytest.raises(dev.SqmcGpuError) as e:
        s.g.orbital_gradient(np.full((norb, norb), np.nan), s.G)
    assert e.value.code == BAD_ARG
    with pytest.raises(ValueError):
        s.g.orbital_gradient(s.D[:4, :4], s.G)
    with pytest.raises(ValueError):
        s.g.orbital_gradient(s.D, s.G, "kappa")
    for make in (lambda: H.HegHost(3, 0.5, 14, 7, 1.49).gpu(), lambda: H.HubbardHost(4, 4, True, 8, 8).gpu(), lambda: H.HubbardKHost(4, 4, 8, 8).gpu()):
        g = make()
        try:
            n = g.norb
            big = [np.full(n * n, 7.25) for _ in range(3)]
            assert _raw(L, g.h, np.zeros(n * n), np.zeros(n ** 4), big) == UNSUPPORTED and all(bool(np.all(a == 7.25)) for a in big)
        finally:
            g.close()
    # a combine_2 the rotation door refuses: refused here by the same test
    c2 = s.host.combine_2.copy()
    c2[1, 2] = c2[3, 3]
    gb = dev.GpuChem(norb, s.host.nup, s.host.ndn, s.host.orbsym, s.host.prod.reshape(-1), c2.reshape(-1), s.host.integrals, n_group=s.host.n_group)
    try:
        assert _raw(L, gb.h, D, G, outs) == UNSUPPORTED and untouched()
        with pytest.raises(dev.SqmcGpuError) as e:
            gb.rotate_integrals(np.eye(norb))
        assert e.value.code == UNSUPPORTED
    finally:
        gb.close()
    # time_sym contexts are accepted (only the integrals are read), and give the bits of the plain context
    ref = s.g.orbital_gradient(s.D, s.G)
    gt = dev.GpuChem(norb, s.host.nup, s.host.ndn, s.host.orbsym, s.host.prod.reshape(-1), s.host.combine_2.reshape(-1), s.host.integrals,
                     n_group=s.host.n_group, time_sym=True, z=1)
    try:
        got = gt.orbital_gradient(s.D, s.G)
        assert all(got[k].tobytes() == ref[k].tobytes() for k in NAMES)
    finally:
        gt.close()
    # a good call afterwards, with an output left out and its pointer null
    assert _raw(L, s.g.h, D, G, [outs[0], None, outs[2]]) == OK and bool(np.all(outs[1] == 7.25))
    assert outs[0].tobytes() == ref["fock"].tobytes(order="F") and outs[2].tobytes() == ref["hdiag"].tobytes(order="F")


def test_every_take_fails_in_turn(dev, tmp_path_factory):
    norb = 5
    s = _system(dev, tmp_path_factory, norb)
    L = s.g.L
    L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]
    L.sqmc_gpu_debug_scratch_fail_at.argtypes = [C.c_int64]

    def counters():
        a = [C.c_int64() for _ in range(4)]
        assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 0) == OK
        return tuple(x.value for x in a)
    D, G = np.ascontiguousarray(s.D.reshape(-1, order="F")), np.ascontiguousarray(s.G.reshape(-1, order="F"))
    outs = [np.full(norb * norb, 7.25) for _ in range(3)]
    base = counters()
    assert _raw(L, s.g.h, D, G, outs) == OK
    first = [a.copy() for a in outs]
    after = counters()
    assert after[:2] == base[:2]
    takes = after[3] - base[3]
    assert 5 <= takes <= 20, takes
    for a in outs:
        a[:] = 7.25
    for k in range(1, takes + 1):
        assert L.sqmc_gpu_debug_scratch_fail_at(k) == OK
        rc = _raw(L, s.g.h, D, G, outs)
        L.sqmc_gpu_debug_scratch_fail_at(0)
        assert rc == ERR_HIP, (k, takes, rc, L.sqmc_gpu_last_error())
        assert counters()[:2] == base[:2], (k, "live allocations after a failed take")
        assert all(bool(np.all(a == 7.25)) for a in outs), (k, "a failed call wrote an output")
        assert _raw(L, s.g.h, D, G, outs) == OK and counters()[:2] == base[:2]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, first)), k
        for a in outs:
            a[:] = 7.25
    print("orbital gradient: %d takes, every early return balanced" % takes)
