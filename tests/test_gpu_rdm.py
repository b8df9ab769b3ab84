"""The 1-RDM entries of the HIP library (sqmc_gpu_hci_1rdm, sqmc_gpu_hci_1rdm_pt), host.hci_one_rdm and the &natorb stage of the deck
runner against tests/rdm_checker.py, which shares nothing with the library.  Every comparison bound is the checker's derived rounding
bound; exact zeros, the HF matrix and the sign cases are compared with ==.  The kernels work in blocks of 256 threads on chunks of
1024 determinants (RDM_T, RDM_CHUNK of sqmc_amd/csrc/rdm_kernels.h): the list sizes below straddle both."""
import io
import math
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import hci_checker as HC          # noqa: E402
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
BAD_ARG, UNSUPPORTED = -1, -3
BLOCK, CHUNK = 256, 1024
SIZES = [1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1]


def _arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


def _normalised(rng, n):
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    s = math.sqrt(math.fsum(x * x for x in c))
    return [x / s for x in c]


def _neighbours(rng, start, norb, n):
    """n distinct determinants grown from start by single-orbital moves of members: a list with many off-diagonal terms"""
    have, lst = {start}, [start]
    while len(lst) < n:
        u, d = lst[rng.randrange(len(lst))]
        spin = rng.randrange(2)
        s = d if spin else u
        occ = RC.occupation(s)
        emp = [r for r in range(norb) if r not in occ]
        if not occ or not emp:
            continue
        s2 = (s ^ (1 << rng.choice(occ))) | (1 << rng.choice(emp))
        det = (u, s2) if spin else (s2, d)
        if det not in have:
            have.add(det); lst.append(det)
    return lst


def _check(g, dets, c, norb, sym=None, tag=""):
    up, dn = _arrays(dets)
    got = g.one_rdm(up, dn, c, sym)
    exp = RC.one_rdm(dets, c, norb, sym)
    fails, worst = RC.compare(exp, got)
    print("%s n = %d: worst |delta| / bound = %.3f" % (tag, len(dets), worst))
    assert not fails, fails[:4]
    return got, exp


@pytest.fixture(scope="module")
def dev():
    import sqmc_amd
    sqmc_amd.set_device(0)
    return sqmc_amd


_CHEM = {}


def _chem(dev, nelec=8, nup=4, **kw):
    """(host, context, checker Hamiltonian) of the C2 fixture, walk conventions (time_sym off), kept for the module"""
    from sqmc_amd import host as H
    key = (nelec, nup, tuple(sorted(kw.items())))
    if key not in _CHEM:
        h = H.ChemHost(FCIDUMP, nelec, nup, "d2h", **kw)
        _CHEM[key] = (h, h.gpu(), PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)]))
    return _CHEM[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for _, g, _ in _CHEM.values():
        g.close()
    _CHEM.clear()


_SD = {}


def _hf_singles_doubles(h):
    if "u" not in _SD:
        hf = (int(h.hf_up), int(h.hf_dn))
        _SD["u"] = sorted(set((int(a), int(b)) for a, b in PC.excitations_chem(hf[0], hf[1], h.norb)) - {hf})
        _SD["singles"] = [d for d in _SD["u"] if PC._pop(d[0] ^ hf[0]) + PC._pop(d[1] ^ hf[1]) == 2]
    return _SD["u"], _SD["singles"]


def _sd_list(h, rng, n):
    """HF, up to 16 of its single excitations and random doubles: n determinants in random order"""
    univ, singles = _hf_singles_doubles(h)
    lst = [(int(h.hf_up), int(h.hf_dn))] + rng.sample(singles, min(16, max(n - 1, 0)))
    pool = [d for d in univ if d not in set(lst)]
    lst += rng.sample(pool, n - len(lst))
    rng.shuffle(lst)
    return lst[:n]


# ---------------------------------------------------------------------------------------------- the variational entry
def test_hf_determinant_is_the_occupation_matrix(dev):
    h, g, _ = _chem(dev)
    got = g.one_rdm([h.hf_up], [h.hf_dn], [1.0])
    want = np.zeros((h.norb, h.norb))
    for p in range(h.norb):
        want[p, p] = (int(h.hf_up) >> p & 1) + (int(h.hf_dn) >> p & 1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_variational_chem(dev, n):
    """C2, 8 electrons in 26 orbitals: random normalised coefficients on HF's singles and doubles; sizes one below, at and one above
    the wavefront (64), the block (256) and the chunk (1024)"""
    h, g, _ = _chem(dev)
    rng = random.Random(1000 + n)
    dets = _sd_list(h, rng, n)
    c = _normalised(rng, n)
    got, exp = _check(g, dets, c, h.norb, tag="chem")
    assert abs(float(np.trace(got)) - 8.0 * math.fsum(x * x for x in c)) <= exp.trace_bound() + 16 * RC.U * 8.0


@pytest.mark.parametrize("nup", [1, 2, 3, 4])
def test_orbital_extremes_sign(dev, nup):
    """two determinants that differ by the move orbital 0 -> orbital norb - 1 of one spin with nup - 1 (up) or ndn - 1 (dn) electrons in
    between: 0 .. 3 over the four contexts for up, 6 .. 3 for dn.  The entry is (-1)^between c_1 c_2, exactly"""
    h, g, _ = _chem(dev, 8, nup)
    norb, last = h.norb, h.norb - 1
    for spin, ne in ((0, nup), (1, 8 - nup)):
        rng = random.Random(10 * nup + spin)
        mid = sum(1 << k for k in rng.sample(range(1, last), ne - 1))
        other = sum(1 << k for k in rng.sample(range(norb), 8 - ne))
        a, b = mid | 1, mid | (1 << last)
        dets = [(a, other), (b, other)] if spin == 0 else [(other, a), (other, b)]
        c = [0.6, -0.8]
        got, _ = _check(g, dets, c, norb, tag="extremes nup=%d spin=%d" % (nup, spin))
        want = (-1.0) ** (ne - 1) * (0.6 * -0.8)
        assert got[0, last] == want and got[last, 0] == want


def test_bit_63_on_the_8x8_lattice(dev):
    from sqmc_amd import host as H
    h = H.HubbardHost(8, 8, True, 3, 2)
    g = h.gpu()
    try:
        a_up, dn0 = (1 << 0) | (1 << 5) | (1 << 9), (1 << 62) | (1 << 3)
        dets = [(a_up, dn0), ((a_up ^ 1) | (1 << 63), dn0), (a_up, (1 << 63) | (1 << 3)), (a_up, (1 << 63) | (1 << 0)),
                ((1 << 62) | (1 << 5) | (1 << 9), dn0), ((1 << 63) | (1 << 62) | (1 << 61), dn0)]
        c = [0.5, -0.4, 0.3, 0.45, -0.35, 0.4]
        got, exp = _check(g, dets, c, 64, tag="bit 63")
        assert exp.count(0, 63) == 1 and got[0, 63] == 0.5 * -0.4 and got[63, 0] == 0.5 * -0.4        # up 0 -> 63 across 5 and 9: +
        assert exp.count(63, 63) == 4 and exp.count(62, 63) == 2 and exp.count(3, 0) == 1
        assert exp.count(0, 62) == 1 and got[0, 62] == 0.5 * -0.35                                      # up 0 -> 62 across 5 and 9
    finally:
        g.close()


@pytest.mark.parametrize("nelec,nup", [(8, 5), (4, 3)])
def test_spin_counts(dev, nelec, nup):
    """nup != ndn, and a sector with one electron of one spin"""
    h, g, _ = _chem(dev, nelec, nup)
    rng = random.Random(nelec * 10 + nup)
    dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 90)
    c = _normalised(rng, len(dets))
    got, exp = _check(g, dets, c, h.norb, tag="nup=%d ndn=%d" % (nup, nelec - nup))
    assert sum(exp.count(p, r) > 0 for p in range(h.norb) for r in range(h.norb) if p != r) > 20


def _refused(fn, code):
    import sqmc_amd
    with pytest.raises(sqmc_amd.SqmcGpuError) as e:
        fn()
    assert e.value.code == code, e.value


def test_list_handling(dev):
    from sqmc_amd import host as H
    h, g, _ = _chem(dev)
    rng = random.Random(77)
    dets = _sd_list(h, rng, 300)
    c = _normalised(rng, 300)
    for k in range(0, 300, 7):
        c[k] = 0.0
    up, dn = _arrays(dets)
    base = g.one_rdm(up, dn, c)
    order = sorted(range(300), key=lambda k: dets[k])
    assert g.one_rdm(up[order], dn[order], np.array(c)[order]).tobytes() == base.tobytes()
    fails, _ = RC.compare(RC.one_rdm(dets, c, h.norb), base)
    assert not fails, fails[:4]
    # refusals leave the output untouched: the binding's buffer starts as zeros, so call the library with a marked one
    import ctypes as C
    marked = np.full(h.norb * h.norb, 7.25)
    L = g.L

    def raw(u, d, cc, ctx=g):
        u, d, cc = np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(d, np.uint64), np.ascontiguousarray(cc, np.float64)
        L.sqmc_gpu_hci_1rdm.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        return L.sqmc_gpu_hci_1rdm(ctx.h, len(u), u.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), None,
                                   marked.ctypes.data_as(C.c_void_p))
    twice = np.concatenate((up, up[41:42])), np.concatenate((dn, dn[41:42])), np.concatenate((c, [0.1]))
    assert raw(*twice) == BAD_ARG and np.all(marked == 7.25)
    _refused(lambda: g.one_rdm(*twice), BAD_ARG)
    wrong = up.copy(); wrong[5] |= np.uint64(1 << 20) if not int(wrong[5]) >> 20 & 1 else np.uint64(1 << 21)
    assert raw(wrong, dn, c) == BAD_ARG and np.all(marked == 7.25)
    _refused(lambda: g.one_rdm(wrong, dn, c), BAD_ARG)
    beyond = up.copy(); beyond[3] = (int(beyond[3]) & ~(1 << PC._bits(int(beyond[3]))[0])) | (1 << 40)
    _refused(lambda: g.one_rdm(beyond, dn, c), BAD_ARG)
    ts = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1)
    gt = ts.gpu()
    try:
        assert raw(up, dn, c, gt) == UNSUPPORTED and np.all(marked == 7.25)
        _refused(lambda: gt.one_rdm(up, dn, c), UNSUPPORTED)
        _refused(lambda: gt.one_rdm_pt(up, dn, c, -76.0, 1e-3), UNSUPPORTED)
    finally:
        gt.close()
    assert g.one_rdm(up, dn, c).tobytes() == base.tobytes()          # an ordinary call after the refusals


def test_filter_by_orbital_symmetry(dev):
    h, g, _ = _chem(dev)
    rng = random.Random(31)
    dets = _sd_list(h, rng, 200)
    c = _normalised(rng, 200)
    sym = [int(x) for x in h.orbsym[1:h.norb + 1]]
    plain, exp = _check(g, dets, c, h.norb, tag="unfiltered")
    cross = [(p, r) for p in range(h.norb) for r in range(h.norb) if sym[p] != sym[r]]
    assert max(abs(exp.value(p, r)) for p, r in cross) > 1e-3
    filt, _ = _check(g, dets, c, h.norb, sym, tag="filtered")
    for p in range(h.norb):
        for r in range(h.norb):
            if sym[p] != sym[r]:
                assert filt[p, r] == 0.0 and not np.signbit(filt[p, r])
            else:
                assert filt[p, r].tobytes() == plain[p, r].tobytes()


def test_other_systems(dev):
    from sqmc_amd import host as H
    for name, h in (("heg", H.HegHost(3, 0.5, 14, 7, 1.49)), ("hubbard2", H.HubbardHost(4, 4, True, 8, 8)), ("hubbardk", H.HubbardKHost(4, 3, 5, 5))):
        g = h.gpu()
        try:
            rng = random.Random(len(name))
            dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 130)
            c = _normalised(rng, len(dets))
            _, exp = _check(g, dets, c, h.norb, tag=name)
            assert sum(exp.count(p, r) > 0 for p in range(h.norb) for r in range(h.norb) if p != r) > 20
        finally:
            g.close()


# ---------------------------------------------------------------------------------------------- the PT entry
_PT = {}


def _pt_case_chem(dev):
    """HF and the nine determinants its strongest paths reach, coefficients 0.9 and +-(0.05 .. 0.2) normalised; eps_pt_big by pick_eps
    keeps half of the distinct screen values"""
    if "chem" not in _PT:
        h, g, HH = _chem(dev)
        if not getattr(g, "_hb_set", False):
            g.set_hb_tables(*h.hb_tables(g)); g._hb_set = True
        hf = (int(h.hf_up), int(h.hf_dn))
        live = sorted((p for p in HC.raw_paths(HH, hf) if not p.noise), key=lambda p: (-abs(p.raw), p.det))
        var = [hf] + [p.det for p in live[:9]]
        rng = random.Random(5)
        co = [0.9] + [rng.choice((-1, 1)) * rng.uniform(0.05, 0.2) for _ in var[1:]]
        _PT["chem"] = _pt_finish(HH, var, co, h.norb, 8) + (g,)
    return _PT["chem"]


def _pt_case_heg(dev):
    """the electron gas has no single excitation inside one momentum sector, so a wavefunction of one sector has no PT term in its
    1-RDM at all; this list mixes sectors: HF and 15 of its single excitations, one from each of the 15 momentum transfers that the
    most (p, r) pairs share, alternating spin.  The single excitations of HF with the same transfers then lie in the connected space"""
    if "heg" not in _PT:
        from sqmc_amd import host as H
        h = H.HegHost(3, 0.5, 14, 7, 1.49)
        HH = PC.HegH(h.k_vectors, h.length_cell)
        hf = (int(h.hf_up), int(h.hf_dn))
        occ = RC.occupation(hf[0])
        sect = {}
        for p in occ:
            for r in range(h.norb):
                if r not in occ:
                    sect.setdefault(tuple(int(x) for x in (h.k_rel[r] - h.k_rel[p])), []).append((p, r))
        var = [hf]
        for k, q in enumerate(sorted(sect, key=lambda q: (-len(sect[q]), q))[:15]):
            p, r = sect[q][0]
            var.append(((hf[0] ^ (1 << p)) | (1 << r), hf[1]) if k % 2 == 0 else (hf[0], (hf[1] ^ (1 << p)) | (1 << r)))
        rng = random.Random(11)
        co = [0.8] + [rng.choice((-1, 1)) * rng.uniform(0.1, 0.2) for _ in var[1:]]
        _PT["heg"] = _pt_finish(HH, var, co, h.norb, 14) + (h.gpu(),)
    return _PT["heg"]


def _pt_finish(HH, var, co, norb, nelec):
    s = math.sqrt(math.fsum(x * x for x in co))
    co = [x / s for x in co]
    vals = HC.screen_values(HH, var, co)
    eps = HC.pick_eps(vals, max(1, len(set(vals)) // 2))
    e_var = min(HC.diagonal(HH, v)[0] for v in var) - 0.1
    first = RC.first_order(HH, var, co, e_var, eps)
    exp, con, n_hit = RC.one_rdm_pt(HH, var, co, e_var, eps, norb, first=first)
    assert not con.borderline and not con.optional
    return var, co, e_var, eps, exp, con, n_hit, RC.one_rdm(var, co, norb), nelec


@pytest.fixture(scope="module", autouse=True)
def _close_pt():
    yield
    if "heg" in _PT:
        _PT["heg"][-1].close()
    _PT.clear()


@pytest.mark.parametrize("which", ["chem", "heg"])
def test_pt_against_the_checker(dev, which):
    var, co, e_var, eps, exp, con, n_hit, var_exp, nelec, g = (_pt_case_chem if which == "chem" else _pt_case_heg)(dev)
    norb = exp.norb
    assert n_hit >= 100, n_hit
    assert max(abs(exp.value(p, r) - var_exp.value(p, r)) for p in range(norb) for r in range(norb) if p != r) > 1e-6
    up, dn = _arrays(var)
    got = {}
    for ns in (1, 3):
        m, n_conn = g.one_rdm_pt(up, dn, co, e_var, eps, ns)
        fails, worst = RC.compare(exp, m)
        print("%s PT, %d slices: %d connected, %d singles outside, worst |delta| / bound = %.3f" % (which, ns, n_conn, n_hit, worst))
        assert not fails, fails[:4]
        assert n_conn == len(con.merged)
        assert abs(float(np.trace(m)) - nelec * math.fsum(x * x for x in co)) <= exp.trace_bound() + 16 * RC.U * nelec
        assert g.one_rdm_pt(up, dn, co, e_var, eps, ns)[0].tobytes() == m.tobytes()
        got[ns] = m
    for p in range(norb):
        for r in range(norb):
            assert abs(got[1][p, r] - got[3][p, r]) <= 2.0 * exp.bound(p, r)
    # the variational part alone, when nothing is connected: eps above every element
    m, n_conn = g.one_rdm_pt(up, dn, co, e_var, 1e6)
    fails, _ = RC.compare(var_exp, m)
    assert not fails and n_conn == len(var)
    order = list(range(len(var)))[::-1]
    assert g.one_rdm_pt(up[order], dn[order], np.array(co)[order], e_var, eps)[0].tobytes() == got[1].tobytes()


def test_pt_refusals(dev):
    from sqmc_amd import host as H
    hk = H.HubbardKHost(4, 4, 2, 2, 1.0, 4.0, space_sym=True, z=1, p=1, start=(17, 3))      # 2 up 2 dn at total momentum 0
    g = hk.gpu()
    try:
        _refused(lambda: g.one_rdm_pt([hk.hf_up], [hk.hf_dn], [1.0], -10.0, 1e-3), UNSUPPORTED)
        _refused(lambda: g.one_rdm([hk.hf_up], [hk.hf_dn], [1.0]), UNSUPPORTED)
    finally:
        g.close()
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    g = h.gpu()                                           # no heat-bath tables: refused as sqmc_gpu_hci_pt2 refuses it
    try:
        _refused(lambda: g.one_rdm_pt([h.hf_up], [h.hf_dn], [1.0], -76.0, 1e-3), BAD_ARG)
        _refused(lambda: g.hci_pt2([h.hf_up], [h.hf_dn], [1.0], -76.0, 1e-3), BAD_ARG)
    finally:
        g.close()


def test_reproducible_bytes(dev):
    h, g, _ = _chem(dev)
    rng = random.Random(9)
    dets = _sd_list(h, rng, 1500)
    c = _normalised(rng, 1500)
    up, dn = _arrays(dets)
    a = g.one_rdm(up, dn, c)
    assert all(g.one_rdm(up, dn, c).tobytes() == a.tobytes() for _ in range(3))


# ---------------------------------------------------------------------------------------------- host layer and deck
@pytest.fixture(scope="module")
def ts_wavefunction(dev):
    """i_1sigma_g conventions, two states, one iteration at eps_var 5e-3: a few hundred time-symmetrised determinants"""
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    g = h.gpu()
    try:
        g.set_hb_tables(*h.hb_tables(g))
        up, dn, w, e, hist = H.hci_variational(h, g, 5e-3, n_states=2, max_iters=1)
    finally:
        g.close()
    assert 50 <= len(up) <= 1500, hist
    return h, up, dn, w, e


def test_host_layer_on_a_time_symmetrised_wavefunction(ts_wavefunction):
    from sqmc_amd import host as H
    h, up, dn, w, e = ts_wavefunction
    sym = [int(x) for x in h.orbsym[1:h.norb + 1]]
    exps = []
    for i in range(2):
        du, dd, dc = H.time_symmetrized_to_dets(up, dn, w[:, i], h.z)
        exps.append(RC.one_rdm(list(zip(du.tolist(), dd.tolist())), dc.tolist(), h.norb, sym))
    one = H.hci_one_rdm(h, up, dn, w[:, 0])
    fails, worst = RC.compare(exps[0], one)
    print("host layer: %d combinations, worst |delta| / bound = %.3f" % (len(up), worst))
    assert not fails, fails[:4]
    two = H.hci_one_rdm(h, up, dn, w)
    second = H.hci_one_rdm(h, up, dn, w[:, 1])
    assert not RC.compare(exps[1], second)[0]
    assert np.array_equal(two, (one + second) / 2)
    for p in range(h.norb):
        for r in range(h.norb):
            b = 0.5 * (exps[0].bound(p, r) + exps[1].bound(p, r)) + 2 * RC.U * abs(two[p, r])
            assert abs(two[p, r] - 0.5 * (exps[0].value(p, r) + exps[1].value(p, r))) <= b
    occ, vec = H.natural_orbitals(one, sym)
    assert abs(occ.sum() - 8.0) < 1e-9 and np.all(occ > -1e-12) and np.all(occ < 2.0 + 1e-12)


def _deck_text(natorb):
    t = open(DECK).read().replace("1e-3  1e-7", "5e-3  1e-5").replace("eps_var_sched=2*2e-3", "eps_var_sched=2*1e-2")
    assert "5e-3  1e-5" in t and "2*1e-2" in t
    return t + ("&natorb get_natorbs=.true. /\n" if natorb else "")


def test_deck_with_natorb(dev, tmp_path):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    (tmp_path / "i_1sigma_g_natorb").write_text(_deck_text(True))
    deck = R.parse_hci_deck((tmp_path / "i_1sigma_g_natorb").read_text())
    assert deck["get_natorbs"] and not deck["use_pt"] and deck["n_states"] == 2
    buf, path = io.StringIO(), str(tmp_path / "rdm.npy")
    res = R.run_hci(deck, FCIDUMP, out=buf, one_rdm_path=path)
    lines = buf.getvalue().splitlines()
    marks = [" Getting natural orbitals from the variational 1-RDM", " Using state-averaged 1-RDM from the lowest           2 states",
             " Computing 1-RDM of state           1", " Computing 1-RDM of state           2", "Computing 1-RDM", "1-RDM:", "Done generating rdm",
             "Eigenvectors of 1RDM:", "Eigenvalues of 1RDM:", R.NATORB_STOP]
    at = [lines.index(m) for m in marks]
    assert at == sorted(at) and len(set(at)) == len(at)
    norb = 26
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    rdm = H.hci_one_rdm(h, res["up"], res["dn"], res["wts"])
    assert np.array_equal(rdm, res["rdm"]) and np.array_equal(np.load(path), rdm)
    i0 = lines.index("1-RDM:")
    assert lines[i0 + 1:i0 + 1 + norb] == H.format_real_matrix(rdm).splitlines()
    occ, vec = H.natural_orbitals(rdm, h.orbsym[1:norb + 1])
    i1 = lines.index("Eigenvectors of 1RDM:")
    assert lines[i1 + 1:i1 + 1 + norb] == H.format_real_matrix(vec).splitlines()
    i2 = lines.index("Eigenvalues of 1RDM:")
    assert lines[i2 + 1:i2 + 4] == H.format_eigenvalues(occ).splitlines()
    assert lines[-1] == R.NATORB_STOP
    assert not any("PT energy lowering" in l or "Total energy" in l for l in lines)
    # the same deck without &natorb: the PT stage and its lines as before, nothing of the 1-RDM
    buf2 = io.StringIO()
    res2 = R.run_hci(R.parse_hci_deck(_deck_text(False)), FCIDUMP, out=buf2)
    txt2 = buf2.getvalue()
    assert res2["ndets"] == res["ndets"] and len(res2["states"]) == 2
    assert "Total energy(1)=" in txt2 and "2nd-order PT energy lowering(2)=" in txt2 and "1-RDM" not in txt2 and "natural orbitals" not in txt2
    iters = [l for l in lines if l.startswith("Iteration")]
    assert iters and iters == [l for l in txt2.splitlines() if l.startswith("Iteration")]


def test_deck_with_natorb_and_pt(dev):
    from sqmc_amd import run as R
    deck = R.parse_hci_deck(_deck_text(True).replace("get_natorbs=.true.", "get_natorbs=.true. use_pt=t").replace("5e-3  1e-5", "5e-3  1e-4"))
    assert deck["use_pt"] and deck["eps_pt_big"] == 0.0 and deck["eps_pt"] == 1e-4
    buf = io.StringIO()
    res = R.run_hci(deck, FCIDUMP, out=buf)
    lines = buf.getvalue().splitlines()
    marks = ["Getting natural orbitals from the lowest-order perturbative correction to the variational 1-RDM", "Computing 1-RDM to lowest nonzero order in PT",
             "PT-corrected 1-RDM:", "Done generating rdm", "Eigenvectors of 1RDM:", "Eigenvalues of 1RDM:", R.NATORB_STOP]
    at = [lines.index(m) for m in marks]
    assert at == sorted(at)
    assert abs(float(np.trace(res["rdm"])) - 8.0) < 1e-9
    assert np.max(np.abs(res["rdm"] - res["rdm"].T)) < 1e-12


def test_heg_deck_with_natorb_is_refused():
    from sqmc_amd import run as R
    deck = R.parse_hci_deck(open(os.path.join(ROOT, "tests", "golden", "heg_e2e_i_det")).read() + "&natorb get_natorbs=t /\n")
    assert deck["get_natorbs"]
    with pytest.raises(SystemExit) as e:
        R.run_hci(deck, out=io.StringIO())
    assert "Natural orbitals only implemented for chem so far" in str(e.value)
