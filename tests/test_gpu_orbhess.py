"""sqmc_gpu_one_index_transform and the resident orbital-optimisation plan (sqmc_gpu_orbopt_*) on the MI355X against
tests/orbhess_checker.py: every packed entry of the transformed table and every entry of the Hessian-vector product at the edge sizes
and on both sides of the kernels' seams within the derived rounding bounds, the exact properties with ==, the links to the diagonal
Hessian and the symmetry of the Hessian, the C2 fixture through the Newton-CG step, the deck runner, the refusals and the scratch."""
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
from tests import orbhess_checker as HC      # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
OK, BAD_ARG, ERR_HIP, UNSUPPORTED = 0, -1, -2, -3
V = C.c_void_p
LD = np.longdouble
# the sizes of test_gpu_orbopt.py (every seam of the Fock plan: 20 | 21 chunks per block, 32 | 33 register tile); 32 | 33 is also the
# register tile of the half pass, and norb (norb + 1) / 2 = 3, 6, 15 (one symmetrising tile), 210, 231, 528, 561 (several, none a
# multiple of the tile).  test_the_sizes_straddle_every_seam holds the list to the kernels' own constants.
SMALL_SIZES = [2, 3, 5]
SEAM_SIZES = [20, 21, 32, 33]
EDGE_SIZES = SMALL_SIZES + SEAM_SIZES
NAMES = ("fock", "gradient", "hdiag")


@pytest.fixture(scope="module")
def dev():
    import sqmc_amd
    sqmc_amd.set_device(0)
    return sqmc_amd


# ------------------------------------------------------------------------------------------------------------------ synthetic systems
_SYS, _CTX = {}, []


class _System:
    pass


def _pack_index(host):
    """(index of (pq|rs) for every p, q, r, s; index of h[p, q]; index of the core energy) in the host's packed table, this test's
    own addressing through combine_2"""
    n1, c2 = host.norb + 1, host.combine_2
    pr = c2[1:n1, 1:n1].astype(np.int64)
    hi, lo = np.maximum(pr[:, :, None, None], pr[None, None, :, :]), np.minimum(pr[:, :, None, None], pr[None, None, :, :])
    A = int(c2[n1, n1])
    return (hi * (hi - 1)) // 2 + lo, A * (A - 1) // 2 + pr, A * (A - 1) // 2 + A


def _system(dev, tmp_path_factory, norb, seed=None, nelec=2, nup=1):
    """seeded random dense integrals, a symmetric D, a G with G[p,q,r,s] = G[r,s,p,q] = G[q,p,s,r], and a c1 chem context that holds the
    integrals; kept for the module together with what the tests compute from it once"""
    from sqmc_amd import host as H
    seed = 7000 + norb if seed is None else seed
    key = (norb, seed)
    if key not in _SYS:
        s = _System()
        s.norb = norb
        s.h, s.e, s.D, s.G = OC.random_system(norb, seed)
        path = str(tmp_path_factory.mktemp("orbhess%d" % norb) / "FCIDUMP")
        with open(path, "w") as f:          # a placeholder with the right header: the integrals come from with_integrals
            f.write(" &FCI NORB=%d,NELEC=%d,MS2=0,\n  ORBSYM=%s,\n  ISYM=1,\n &END\n" % (norb, nelec, ",".join(["1"] * norb)))
            f.write("".join("%.17e %d %d 0 0\n" % (0.5 + p, p + 1, p + 1) for p in range(norb)) + "%.17e 0 0 0 0\n" % -1.5)
        base = H.ChemHost(path, nelec, nup, "c1")
        s.i2, s.i1, s.icore = _pack_index(base)
        packed = np.zeros_like(base.integrals)
        packed[s.i2] = s.e; packed[s.i1] = s.h; packed[s.icore] = -1.5
        s.host = base.with_integrals(packed)
        s.g = s.host.gpu()
        _CTX.append(s.g)
        s.kappa = HC.random_kappa(norb, 8000 + norb)
        s.plan = s.g.orbopt_plan(s.D, s.G)
        s.sigma = s.plan.hessian_vector(s.kappa)
        s.fabs0 = OC.fock_abs(s.h, s.e, s.D, s.G)
        _SYS[key] = s
    return _SYS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for s in _SYS.values():
        s.plan.close()
    for g in _CTX:
        g.close()
    _CTX.clear(); _SYS.clear()


def _exact(sig):
    assert np.array_equal(sig, -sig.T) and np.all(np.diag(sig) == 0.0) and not np.signbit(sig[sig == 0.0]).any()


def _gradient64(s):
    """the gradient at kappa = 0 as a double-precision sum of this test's own (numpy)"""
    n = s.norb
    F = s.h @ s.D.T + s.e.transpose(0, 2, 1, 3).reshape(n, n ** 3) @ s.G.reshape(n, n ** 3).T
    return 2.0 * (F - F.T)


# ----------------------------------------------------------------------------------------------------------------------------- tests
def test_the_sizes_straddle_every_seam(dev):
    """the sizes at which the half pass changes its register tile, and pair counts on both sides of one symmetrising tile and off
    its multiples, from the library's own plan"""
    L = dev.load_library()
    L.sqmc_gpu_debug_orbhess_plan.argtypes = [C.c_int32, V]
    plans = {}
    for n in range(1, 65):
        out = (C.c_int64 * 4)()
        assert L.sqmc_gpu_debug_orbhess_plan(n, out) == OK
        plans[n] = tuple(out)                          # (register tile, symmetrising tile, pairs, symmetrising blocks)
    assert L.sqmc_gpu_debug_orbhess_plan(0, (C.c_int64 * 4)()) == BAD_ARG and L.sqmc_gpu_debug_orbhess_plan(65, (C.c_int64 * 4)()) == BAD_ARG
    tile = [n for n in range(2, 65) if plans[n][0] != plans[n - 1][0]]
    assert tile == [33] and all(n in SEAM_SIZES and n - 1 in SEAM_SIZES for n in tile)
    ts = plans[2][1]
    assert all(plans[n][2] == n * (n + 1) // 2 for n in plans)
    assert any(plans[n][3] == 1 for n in EDGE_SIZES) and any(plans[n][3] > 1 for n in EDGE_SIZES)        # one tile, and several
    assert all(plans[n][2] % ts for n in EDGE_SIZES)                                                      # a ragged last tile everywhere
    assert plans[64][2] == 2080 and plans[64][3] == 65 * 66 // 2


@pytest.mark.parametrize("norb", EDGE_SIZES)
def test_one_index_transform_every_entry(dev, tmp_path_factory, norb):
    """a general (not antisymmetric) kappa: every packed entry against the checker's literal statement, the slots no pair addresses
    and the core slot 0.0, exact linearity under a factor 2, and +0.0 throughout for kappa = 0"""
    s = _system(dev, tmp_path_factory, norb)
    k = HC.random_kappa(norb, 8100 + norb, antisymmetric=False)
    assert not np.array_equal(k, -k.T)
    out = s.g.one_index_transform(k)
    assert out.shape == s.host.integrals.shape and out.dtype == np.float64
    ht, et = HC.one_index_literal(s.h, s.e, k)
    a1, a2 = HC.one_index_abs(s.h, s.e, k)
    b1, b2 = HC.one_index_bound(norb, a1, a2)
    d1, d2 = np.abs(out[s.i1] - np.asarray(ht, float)), np.abs(out[s.i2] - np.asarray(et, float))
    print("norb = %d: worst |delta| / bound: one-body %.4f, two-body %.4f" % (norb, float(np.max(d1 / b1)), float(np.max(d2 / b2))))
    assert np.all(d1 <= b1) and np.all(d2 <= b2)
    rest = np.ones(len(out), bool)
    rest[s.i2.reshape(-1)] = False; rest[s.i1.reshape(-1)] = False
    assert rest[s.icore] and rest.sum() >= 2 and np.all(out[rest] == 0.0)
    assert not np.signbit(out[out == 0.0]).any()
    assert s.g.one_index_transform(2.0 * k).tobytes() == (2.0 * out).tobytes()
    assert s.g.one_index_transform(k).tobytes() == out.tobytes()
    zero = s.g.one_index_transform(np.zeros((norb, norb)))
    assert not zero.any() and not np.signbit(zero).any()


@pytest.mark.parametrize("norb", SMALL_SIZES)
def test_sigma_is_the_second_derivative_of_the_energy(dev, tmp_path_factory, norb):
    """every entry against the value read off the rotated energies, and against the host yardstick"""
    from sqmc_amd import host as H
    s = _system(dev, tmp_path_factory, norb)
    _exact(s.sigma)
    want = HC.sigma_from_energy(s.h, s.e, s.D, s.G, s.kappa)
    g = np.asarray(2 * (OC.fock_literal(s.h, s.e, s.D, s.G) - OC.fock_literal(s.h, s.e, s.D, s.G).T), float)
    b = HC.sigma_bound(norb, s.h, s.e, s.D, s.G, s.kappa, g, s.fabs0)
    d = np.abs(s.sigma - np.asarray(want, float))
    off = ~np.eye(norb, dtype=bool)
    print("norb = %d: worst |delta sigma| / bound = %.4f, max|sigma| = %.3e" % (norb, float(np.max(d[off] / b[off])), float(np.max(np.abs(s.sigma)))))
    assert np.all(d[off] <= b[off]) and np.max(np.abs(s.sigma)) > 1e-3
    ref = H.orbital_hessian_vector_host(s.host, s.D, s.G, s.kappa)
    assert np.all(np.abs(s.sigma - ref)[off] <= 2 * b[off])
    assert np.array_equal(H.dense_integrals(s.host)[1], s.e)


@pytest.mark.parametrize("norb", SEAM_SIZES)
def test_sigma_at_the_seams(dev, tmp_path_factory, norb):
    """every entry against the checker's literal statement in longdouble"""
    s = _system(dev, tmp_path_factory, norb)
    _exact(s.sigma)
    want = np.asarray(HC.sigma_literal(s.h, s.e, s.D, s.G, s.kappa), float)
    b = HC.sigma_bound(norb, s.h, s.e, s.D, s.G, s.kappa, _gradient64(s), s.fabs0)
    off = ~np.eye(norb, dtype=bool)
    d = np.abs(s.sigma - want)
    print("norb = %d: worst |delta sigma| / bound = %.4f" % (norb, float(np.max(d[off] / b[off]))))
    assert np.all(d[off] <= b[off])


def test_64_orbitals_on_a_sample(dev, tmp_path_factory):
    norb = 64
    s = _system(dev, tmp_path_factory, norb)
    _exact(s.sigma)
    rng = np.random.default_rng(64)
    g = _gradient64(s)
    b = HC.sigma_bound(norb, s.h, s.e, s.D, s.G, s.kappa, g, s.fabs0, g_factor=2.0)
    pairs = [(0, 1), (0, 63), (31, 32), (62, 63)] + [tuple(sorted(int(x) for x in rng.choice(norb, 2, replace=False))) for _ in range(2)]
    worst = 0.0
    for (p, q), want in HC.sigma_literal_entries(s.h, s.e, s.D, s.G, s.kappa, pairs, g).items():
        d = abs(s.sigma[p, q] - float(want))
        assert d <= b[p, q], (p, q, d, b[p, q])
        worst = max(worst, d / b[p, q])
    # the transformed table on a sample of entries
    k = HC.random_kappa(norb, 8164, antisymmetric=False)
    out = s.g.one_index_transform(k)
    w2 = 0.0
    for P, Q, R, S in [(0, 0, 0, 0), (63, 63, 63, 63), (63, 0, 31, 32), (5, 5, 60, 2)] + [tuple(int(x) for x in rng.integers(0, norb, 4)) for _ in range(20)]:
        want = HC.one_index_entry(s.e, k, P, Q, R, S)
        ak = np.abs(k)
        a2 = float(np.sum(ak[:, P] * np.abs(s.e[:, Q, R, S])) + np.sum(ak[:, Q] * np.abs(s.e[P, :, R, S])) + np.sum(ak[:, R] * np.abs(s.e[P, Q, :, S]))
                   + np.sum(ak[:, S] * np.abs(s.e[P, Q, R, :])))
        d, bb = abs(out[s.i2[P, Q, R, S]] - float(want)), (4 * norb + 2) * HC.U53 * a2
        assert d <= bb, (P, Q, R, S, d, bb)
        w2 = max(w2, d / bb)
    assert out[s.icore] == 0.0
    print("norb = 64: worst |delta| / bound: sigma %.4f, transformed integrals %.4f" % (worst, w2))


@pytest.mark.parametrize("norb", [5, 21, 33])
def test_exact_properties_and_the_same_bits_again(dev, tmp_path_factory, norb):
    s = _system(dev, tmp_path_factory, norb)
    _exact(s.sigma)
    assert s.plan.hessian_vector(s.kappa).tobytes() == s.sigma.tobytes()
    assert s.plan.hessian_vector(2.0 * s.kappa).tobytes() == (2.0 * s.sigma).tobytes()
    zero = s.plan.hessian_vector(np.zeros((norb, norb)))
    assert not zero.any() and not np.signbit(zero).any()
    ref = s.g.orbital_gradient(s.D, s.G)
    got = s.plan.gradient()
    assert sorted(got) == sorted(NAMES) and all(got[k].tobytes() == ref[k].tobytes() for k in NAMES)
    assert list(s.plan.gradient("hdiag")) == ["hdiag"] and s.plan.gradient("hdiag")["hdiag"].tobytes() == ref["hdiag"].tobytes()
    with s.g.orbopt_plan(s.D, s.G) as p2:
        assert p2.hessian_vector(s.kappa).tobytes() == s.sigma.tobytes()
        assert all(p2.gradient()[k].tobytes() == ref[k].tobytes() for k in NAMES)
    assert p2.h is None
    g2 = s.host.gpu()
    try:
        with g2.orbopt_plan(s.D, s.G) as p3:
            assert p3.hessian_vector(s.kappa).tobytes() == s.sigma.tobytes()
    finally:
        g2.close()


def test_links_to_the_diagonal_hessian_and_the_symmetry_of_the_hessian(dev, tmp_path_factory):
    norb = 5
    s = _system(dev, tmp_path_factory, norb)
    hd = s.plan.gradient("hdiag")["hdiag"]
    g = _gradient64(s)
    pairs = [(p, q) for p in range(norb) for q in range(norb) if p != q]
    habs = OC.hdiag_abs(s.h, s.e, s.D, s.G, pairs, s.fabs0)
    for p, q in pairs:
        k = np.asarray(HC.K(norb, p, q), float)
        sig = s.plan.hessian_vector(k)
        bound = HC.sigma_bound(norb, s.h, s.e, s.D, s.G, k, g, s.fabs0)[p, q] + OC.hdiag_bound(norb, habs[(p, q)])
        assert abs(sig[p, q] - hd[p, q]) <= bound, (p, q)
    lam = HC.random_kappa(norb, 8205)
    s_l = s.plan.hessian_vector(lam)
    b_k, b_l = HC.sigma_bound(norb, s.h, s.e, s.D, s.G, s.kappa, g, s.fabs0), HC.sigma_bound(norb, s.h, s.e, s.D, s.G, lam, g, s.fabs0)
    up = np.triu(np.ones((norb, norb), bool), 1)
    dot = lambda a, b: float(np.sum(np.asarray(a[up], LD) * np.asarray(b[up], LD)))
    assert abs(dot(s.kappa, s_l) - dot(lam, s.sigma)) <= float(np.sum(np.abs(s.kappa[up]) * b_l[up]) + np.sum(np.abs(lam[up]) * b_k[up]))
    assert abs(dot(s.kappa, s_l)) > 1.0


# ----------------------------------------------------------------------------------------------------------------------- C2 fixture
@pytest.fixture(scope="module")
def c2(dev):
    """the wavefunction of test_gpu_orbopt.py's c2 fixture: C2 cc-pVDZ, 8 electrons in 26 orbitals, d2h, two states after one
    iteration at eps_var 5e-3, the density matrices of state 1 and a context"""
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", hf_symmetry=1)
    g = h.gpu()
    _CTX.append(g)
    g.set_hb_tables(*h.hb_tables(g))
    up, dn, w, e, hist = H.hci_variational(h, g, 5e-3, n_states=2, max_iters=1)
    assert 50 <= len(up) <= 3000, hist
    s = _System()
    s.h, s.g, s.up, s.dn, s.w, s.e = h, g, up, dn, np.asarray(w, float).reshape(len(up), -1), e
    s.D = H.hci_one_rdm(h, up, dn, s.w[:, 0])
    s.G = H.spin_free_two_rdm(H.hci_two_rdm(h, up, dn, s.w[:, 0]))
    s.sym = np.asarray(h.orbsym[1:h.norb + 1])
    return s


def test_c2_sigma_is_zero_between_irreps(c2):
    from sqmc_amd import host as H
    og = c2.g.orbital_gradient(c2.D, c2.G)
    kappa = H.orbital_step(og["gradient"], og["hdiag"], c2.sym)
    with c2.g.orbopt_plan(c2.D, c2.G) as plan:
        sig = plan.hessian_vector(kappa)
    _exact(sig)
    diff = c2.sym[:, None] != c2.sym[None, :]
    assert diff.any() and np.all(sig[diff] == 0.0) and np.max(np.abs(sig[~diff])) > 1e-4
    n = c2.h.norb
    dh, de, _ = OC.read_fcidump_dense(FCIDUMP, [int(c2.h.orb_order[i]) for i in range(1, n + 1)])
    b = HC.sigma_bound(n, dh, de, c2.D, c2.G, kappa, og["gradient"])
    ref = H.orbital_hessian_vector_host(c2.h, c2.D, c2.G, kappa)
    assert np.all(np.abs(sig - ref) <= 2 * b)


def test_c2_newton_step_lowers_the_energy_and_the_diagonal_step_is_unchanged(c2):
    from sqmc_amd import host as H
    h, n = c2.h, c2.h.norb
    r = H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, 0], solver="newton")
    assert r["energy_after"] < r["energy_before"] and 0.0 < r["scale"] <= 1.0 and 0.0 < r["max_kappa"] <= H.ORBOPT_MAX_STEP
    assert r["solver"] == "newton" and r["predicted_change"] < 0.0 and 1 <= r["cg_iterations"] <= H.ORBOPT_MAX_CG
    assert r["cg_stop"] in ("converged", "negative_curvature", "max_iterations")
    U = r["rotation"]
    assert np.max(np.abs(U.T @ U - np.eye(n))) <= n * 2.0 ** -50 and np.all(U[c2.sym[:, None] != c2.sym[None, :]] == 0.0)
    # the default is the diagonal step, composed as it always was from the door, orbital_step and the rotation door
    d0 = H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, 0])
    d1 = H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, 0], solver="diagonal")
    keys = {"rotation", "integrals", "energy_before", "energy_after", "max_gradient", "gradient_norm", "max_kappa", "scale", "one_rdm", "two_rdm_sf", "gradient", "hdiag"}
    assert set(d0) == set(d1) == keys
    for k in keys:
        assert np.asarray(d0[k]).tobytes() == np.asarray(d1[k]).tobytes(), k
    og = c2.g.orbital_gradient(c2.D, c2.G, ("gradient", "hdiag"))
    kappa = H.orbital_step(og["gradient"], og["hdiag"], c2.sym)
    assert d0["gradient"].tobytes() == og["gradient"].tobytes() and d0["hdiag"].tobytes() == og["hdiag"].tobytes()
    assert d0["rotation"].tobytes() == H.rotation_from_kappa(d0["scale"] * kappa).tobytes()
    assert d0["integrals"].tobytes() == c2.g.rotate_integrals(d0["rotation"]).tobytes()
    assert r["gradient"].tobytes() == d0["gradient"].tobytes() and r["hdiag"].tobytes() == d0["hdiag"].tobytes()
    print("C2: diagonal step %.3e at scale %g; Newton-CG step %.3e at scale %g (%d products, %s, predicted %.3e)"
          % (d0["energy_after"] - d0["energy_before"], d0["scale"], r["energy_after"] - r["energy_before"], r["scale"], r["cg_iterations"], r["cg_stop"],
             r["predicted_change"]))
    with pytest.raises(ValueError):
        H.optimize_orbitals_step(h, c2.up, c2.dn, c2.w[:, 0], solver="bfgs")


# ----------------------------------------------------------------------------------------------------------------------------- deck
def _deck_text():
    t = open(DECK).read().replace("1e-3  1e-7", "5e-3  1e-5").replace("eps_var_sched=2*2e-3", "eps_var_sched=2*1e-2")
    assert "5e-3  1e-5" in t and "2*1e-2" in t
    return t


def test_deck_with_the_newton_solver(dev, tmp_path, monkeypatch):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    monkeypatch.chdir(tmp_path)
    buf = io.StringIO()
    res = R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=buf, optimize_orbitals=True, orbopt_solver="newton")
    lines = buf.getvalue().splitlines()
    first = "Orbital optimisation: one Newton-CG step from the 1-RDM and the 2-RDM of the variational wavefunction"
    name = H.optorb_fcidump_name(5e-3)
    assert name.startswith("FCIDUMP_opt_eps_var=") and os.path.exists(str(tmp_path / name))
    i0, i1 = lines.index(first), lines.index("Rotated integrals written to " + name)
    assert i1 == i0 + 7 and lines[i0 - 1] == ""
    assert lines[i0 + 2].startswith(" max|g| =") and lines[i0 + 3].startswith(" Hessian-vector products =") and "stopped on: " in lines[i0 + 3]
    assert lines[i0 + 4].startswith(" max|kappa| =") and lines[i0 + 5].startswith(" Fixed-coefficient energy after the step =")
    assert lines[i0 + 6].startswith(" Predicted change =") and "actual change =" in lines[i0 + 6]
    o = res["optimize_orbitals"]
    assert o["energy_after"] < o["energy_before"] and o["solver"] == "newton" and o["predicted_change"] < 0.0 and o["cg_iterations"] >= 1
    # without the solver flag: today's lines
    buf2, path2 = io.StringIO(), str(tmp_path / "FCIDUMP_diag")
    res2 = R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=buf2, optimize_orbitals=path2)
    plain = buf2.getvalue().splitlines()
    j0 = plain.index("Orbital optimisation: one diagonal-Newton step from the 1-RDM and the 2-RDM of the variational wavefunction")
    assert plain.index("Rotated integrals written to " + path2) == j0 + 5 and "Hessian-vector" not in buf2.getvalue()
    assert "solver" not in res2["optimize_orbitals"] and plain[:j0] == lines[:i0]
    assert R.main.__module__ == "sqmc_amd.run"
    with pytest.raises(SystemExit):
        R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=io.StringIO(), orbopt_solver="newton")      # the solver needs --optimize-orbitals


# ------------------------------------------------------------------------------------------------------------- refusals and scratch
def _lib(g):
    L = g.L
    L.sqmc_gpu_one_index_transform.argtypes = [V] * 3
    L.sqmc_gpu_orbopt_prepare.argtypes = [V] * 4
    L.sqmc_gpu_orbopt_gradient.argtypes = [V] * 4
    L.sqmc_gpu_orbopt_hessian_vector.argtypes = [V] * 3
    L.sqmc_gpu_orbopt_free.argtypes = [V]
    L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]
    L.sqmc_gpu_debug_scratch_fail_at.argtypes = [C.c_int64]
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(V)


def test_refusals_leave_the_outputs_untouched(dev, tmp_path_factory):
    from sqmc_amd import host as H
    norb = 5
    s = _system(dev, tmp_path_factory, norb)
    L = _lib(s.g)
    D, G = np.ascontiguousarray(s.D.reshape(-1, order="F")), np.ascontiguousarray(s.G.reshape(-1, order="F"))
    k = np.ascontiguousarray(s.kappa)
    tab, sig = np.full(len(s.host.integrals), 7.25), np.full(norb * norb, 7.25)
    plan = C.c_void_p(12345)
    clean = lambda: bool(np.all(tab == 7.25)) and bool(np.all(sig == 7.25)) and plan.value == 12345
    # nulls
    assert L.sqmc_gpu_one_index_transform(None, _ptr(k), _ptr(tab)) == BAD_ARG and L.sqmc_gpu_one_index_transform(s.g.h, None, _ptr(tab)) == BAD_ARG
    assert L.sqmc_gpu_one_index_transform(s.g.h, _ptr(k), None) == BAD_ARG
    assert L.sqmc_gpu_orbopt_prepare(None, _ptr(D), _ptr(G), C.byref(plan)) == BAD_ARG and L.sqmc_gpu_orbopt_prepare(s.g.h, None, _ptr(G), C.byref(plan)) == BAD_ARG
    assert L.sqmc_gpu_orbopt_prepare(s.g.h, _ptr(D), None, C.byref(plan)) == BAD_ARG and L.sqmc_gpu_orbopt_prepare(s.g.h, _ptr(D), _ptr(G), None) == BAD_ARG
    assert L.sqmc_gpu_orbopt_hessian_vector(None, _ptr(k), _ptr(sig)) == BAD_ARG and L.sqmc_gpu_orbopt_hessian_vector(s.plan.h, None, _ptr(sig)) == BAD_ARG
    assert L.sqmc_gpu_orbopt_hessian_vector(s.plan.h, _ptr(k), None) == BAD_ARG
    assert L.sqmc_gpu_orbopt_gradient(None, _ptr(sig), None, None) == BAD_ARG and L.sqmc_gpu_orbopt_gradient(s.plan.h, None, None, None) == BAD_ARG
    assert L.sqmc_gpu_orbopt_free(None) == OK and clean()
    # non-finite entries; a kappa that is not antisymmetric goes through the transformation and is refused by the product
    for bad in (np.nan, np.inf, -np.inf):
        kb = k.copy(); kb[1, 3] = bad; kb[3, 1] = -bad
        assert L.sqmc_gpu_one_index_transform(s.g.h, _ptr(kb), _ptr(tab)) == BAD_ARG and L.sqmc_gpu_orbopt_hessian_vector(s.plan.h, _ptr(kb), _ptr(sig)) == BAD_ARG
        for which in (0, 1):
            d, gg = D.copy(), G.copy()
            (d, gg)[which][-1] = bad
            assert L.sqmc_gpu_orbopt_prepare(s.g.h, _ptr(d), _ptr(gg), C.byref(plan)) == BAD_ARG
        assert clean()
    for change in (lambda a: a.__setitem__((1, 3), a[1, 3] + 2.0 ** -40), lambda a: a.__setitem__((2, 2), 1e-300)):
        kb = k.copy(); change(kb)
        assert L.sqmc_gpu_orbopt_hessian_vector(s.plan.h, _ptr(kb), _ptr(sig)) == BAD_ARG and clean()
        assert L.sqmc_gpu_one_index_transform(s.g.h, _ptr(kb), _ptr(tab)) == OK and not np.all(tab == 7.25)
        tab[:] = 7.25
    with pytest.raises(dev.SqmcGpuError) as e:
        s.plan.hessian_vector(np.triu(np.ones((norb, norb)), 1))
    assert e.value.code == BAD_ARG
    with pytest.raises(ValueError):
        s.plan.hessian_vector(s.kappa[:4, :4])
    with pytest.raises(ValueError):
        s.g.one_index_transform(s.kappa[:4, :4])
    with pytest.raises(ValueError):
        s.g.orbopt_plan(s.D[:4, :4], s.G)
    with pytest.raises(ValueError):
        s.plan.gradient("kappa")
    # the refused products left the plan usable
    assert s.plan.hessian_vector(s.kappa).tobytes() == s.sigma.tobytes()
    # contexts without an integral table
    for make in (lambda: H.HegHost(3, 0.5, 14, 7, 1.49).gpu(), lambda: H.HubbardHost(4, 4, True, 8, 8).gpu(), lambda: H.HubbardKHost(4, 4, 8, 8).gpu()):
        g = make()
        try:
            n = g.norb
            big = np.full(4096, 7.25)
            assert L.sqmc_gpu_one_index_transform(g.h, _ptr(np.zeros(n * n)), _ptr(big)) == UNSUPPORTED and bool(np.all(big == 7.25))
            assert L.sqmc_gpu_orbopt_prepare(g.h, _ptr(np.zeros(n * n)), _ptr(np.zeros(n ** 4)), C.byref(plan)) == UNSUPPORTED and clean()
        finally:
            g.close()
    # a combine_2 the rotation door refuses
    c2 = s.host.combine_2.copy()
    c2[1, 2] = c2[3, 3]
    gb = dev.GpuChem(norb, s.host.nup, s.host.ndn, s.host.orbsym, s.host.prod.reshape(-1), c2.reshape(-1), s.host.integrals, n_group=s.host.n_group)
    try:
        assert L.sqmc_gpu_one_index_transform(gb.h, _ptr(k), _ptr(tab)) == UNSUPPORTED
        assert L.sqmc_gpu_orbopt_prepare(gb.h, _ptr(D), _ptr(G), C.byref(plan)) == UNSUPPORTED and clean()
    finally:
        gb.close()


def test_every_take_fails_in_turn(dev, tmp_path_factory):
    norb = 5
    s = _system(dev, tmp_path_factory, norb)
    L = _lib(s.g)

    def counters():
        a = [C.c_int64() for _ in range(4)]
        assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 0) == OK
        return tuple(x.value for x in a)
    D, G = np.ascontiguousarray(s.D.reshape(-1, order="F")), np.ascontiguousarray(s.G.reshape(-1, order="F"))
    k = np.ascontiguousarray(s.kappa)
    tab, sig = np.full(len(s.host.integrals), 7.25), np.full(norb * norb, 7.25)
    base = counters()

    def prepare():
        plan = C.c_void_p(12345)
        rc = L.sqmc_gpu_orbopt_prepare(s.g.h, _ptr(D), _ptr(G), C.byref(plan))
        if rc == OK:
            assert counters()[0] > base[0]
            out = np.zeros(norb * norb)
            assert L.sqmc_gpu_orbopt_hessian_vector(plan, _ptr(k), _ptr(out)) == OK and out.tobytes() == s.sigma.tobytes(order="F")
            assert L.sqmc_gpu_orbopt_free(plan) == OK
        else:
            assert plan.value == 12345
        return rc
    doors = {"prepare": (prepare, lambda: True),
             "hessian_vector": (lambda: L.sqmc_gpu_orbopt_hessian_vector(s.plan.h, _ptr(k), _ptr(sig)), lambda: bool(np.all(sig == 7.25))),
             "one_index_transform": (lambda: L.sqmc_gpu_one_index_transform(s.g.h, _ptr(k), _ptr(tab)), lambda: bool(np.all(tab == 7.25)))}
    want = s.g.one_index_transform(k)
    for name, (call, untouched) in doors.items():
        before = counters()
        assert call() == OK and counters()[:2] == base[:2]
        takes = counters()[3] - before[3] - (2 if name == "prepare" else 0)       # prepare's good call also ran one product: two takes
        assert {"prepare": 10, "hessian_vector": 2, "one_index_transform": 4}[name] == takes, (name, takes)
        tab[:] = 7.25; sig[:] = 7.25
        for j in range(1, takes + 1):
            assert L.sqmc_gpu_debug_scratch_fail_at(j) == OK
            rc = call()
            L.sqmc_gpu_debug_scratch_fail_at(0)
            assert rc == ERR_HIP, (name, j, rc, L.sqmc_gpu_last_error())
            assert counters()[:2] == base[:2], (name, j, "live allocations after a failed take")
            assert untouched(), (name, j, "a failed call wrote an output")
            assert call() == OK and counters()[:2] == base[:2]
            if name == "hessian_vector":
                assert sig.tobytes() == s.sigma.tobytes(order="F")
            if name == "one_index_transform":
                assert tab.tobytes() == want.tobytes()
            tab[:] = 7.25; sig[:] = 7.25
        print("%s: %d takes, every early return balanced" % (name, takes))
