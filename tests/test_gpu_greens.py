"""The Green's function entry of the HIP library (sqmc_gpu_hci_greens_function), host.hci_greens_function and the &greens_function stage
of the deck runner against tests/greens_checker.py, which shares nothing with the library.  Every comparison bound is the checker's
derived per-entry bound (and the checker asserts that it stays below 1e-8 of the entry's sum of |terms|); structural zeros are compared
with ==.  The kernels work in blocks of 256 threads (GF_T) on chunks of 1024 determinants (GF_CHUNK) and on frequency tiles of 256
(GF_WTILE of sqmc_amd/csrc/greens_kernels.h): the list sizes and the 257-point grid below straddle them."""
import ctypes as C
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
from tests import greens_checker as GC       # noqa: E402
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
BAD_ARG, UNSUPPORTED = -1, -3
T, CHUNK, WTILE = 256, 1024, 256
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, CHUNK - 1, CHUNK, CHUNK + 1]
PARTS = ((GC.NP1, 0), (GC.NM1, 1))


def _arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


def _normalised(rng, n):
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    s = math.sqrt(math.fsum(x * x for x in c))
    return [x / s for x in c]


def _neighbours(rng, start, norb, n):
    """n distinct determinants grown from start by single-orbital moves of members (as tests/test_gpu_rdm.py grows them): many terms
    off the diagonal.  The list of length n is a prefix of every longer one of the same seed"""
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


def _e0(HH, h):
    """an energy a little below the HF determinant's, as a variational energy is"""
    return HH.element(int(h.hf_up), int(h.hf_dn), int(h.hf_up), int(h.hf_dn))[0] - 0.05


def _compare(chk, part, signed, w, got, tag):
    fails, worst = chk.compare(part, signed, w, got)
    print("%s %s %s: %d frequencies, worst |delta| / bound = %.3f" % (tag, part, "signed" if signed else "unsigned", len(w), worst))
    assert not fails, fails[:4]


def _check_both(g, chk, dets, c, e0, w, tag):
    """one call per sign mode with both outputs; returns {signed: (G_np1, G_nm1)}"""
    up, dn = _arrays(dets)
    out = {}
    for signed in (False, True):
        out[signed] = g.greens_function(up, dn, c, e0, w, signed)
        for part, k in PARTS:
            _compare(chk, part, signed, w, out[signed][k], tag)
    return out


_GROWN = {}


def _grown(h, n):
    if "l" not in _GROWN:
        _GROWN["l"] = _neighbours(random.Random(1), (int(h.hf_up), int(h.hf_dn)), h.norb, max(SIZES))
    return _GROWN["l"][:n]


# ---------------------------------------------------------------------------------------------- 1. list sizes
@pytest.mark.parametrize("n", SIZES)
def test_list_sizes(dev, n):
    """C2, 8 electrons in 26 orbitals, lists grown from HF (seed 1): sizes one below, at and one above the wavefront, the block and the
    chunk.  Each half at two frequencies outside its poles, and for n <= 65 and CHUNK + 1 also at the midpoints of its widest interior
    gaps: three of them, or as many as the half's pole list has with 2 * 0.05 Ha of room (the pole list of one or two determinants has
    fewer than three such gaps: HF alone has three distinct N-1 poles and one wide gap among its N+1 poles; from 63 determinants on
    there are three).  The count comes from the checker's pole list, never from the library"""
    h, g, HH = _chem(dev)
    dets = _grown(h, n)
    c = _normalised(random.Random(2000 + n), n)
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, dets, c, e0, h.norb)
    print("n = %d: largest H_mm rounding bound %.2e" % (n, chk.max_h_bound()))
    up, dn = _arrays(dets)
    for part, k in PARTS:
        poles = chk.poles(part)
        w = GC.outside(poles, 0.5)
        if n <= 65 or n == CHUNK + 1:
            ng = min(3, GC.wide_gaps(poles))
            assert ng >= (3 if n >= 63 else 1)
            w = w + GC.in_gaps(poles, ng)
        for signed in (False, True):
            got = g.greens_function(up, dn, c, e0, w, signed, parts=part)
            assert got[1 - k] is None
            _compare(chk, part, signed, w, got[k], "n = %d" % n)


# ---------------------------------------------------------------------------------------------- 2. HF alone
def test_hf_alone(dev):
    h, g, HH = _chem(dev)
    hf = (int(h.hf_up), int(h.hf_dn))
    assert hf[0] == hf[1]
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, [hf], [1.0], e0, h.norb)
    w = GC.outside(chk.all_poles(), 0.4) + GC.in_gaps(chk.poles(GC.NP1), 1)
    out = _check_both(g, chk, [hf], [1.0], e0, w, "HF")
    gp, gm = out[False]
    occ = RC.occupation(hf[0])
    assert len(occ) == 4
    for p in range(h.norb):
        for q in range(h.norb):
            for m in (gp, gm):
                if p != q:
                    assert np.all(m[:, p, q] == 0.0) and not np.any(np.signbit(m[:, p, q]))
        assert np.all((gp if p in occ else gm)[:, p, p] == 0.0)
        assert np.all((gm if p in occ else gp)[:, p, p] != 0.0)
    assert out[True][0].tobytes() == gp.tobytes() and out[True][1].tobytes() == gm.tobytes()


# ---------------------------------------------------------------------------------------------- 3. sign cases
@pytest.mark.parametrize("nup", [1, 2, 3, 4])
def test_orbital_extremes_sign(dev, nup):
    """two determinants that differ by one spin's electron moved orbital 0 -> orbital norb - 1 with nup - 1 (up) or ndn - 1 (dn) electrons
    in between.  Unsigned: the (0, last) and (last, 0) entries of the N-1 part are positive multiples of c_1 c_2 above all poles (one term
    each, a positive denominator); signed: they carry the checker's sign"""
    h, g, HH = _chem(dev, 8, nup)
    norb, last = h.norb, h.norb - 1
    e0 = _e0(HH, h)
    for spin, ne in ((0, nup), (1, 8 - nup)):
        rng = random.Random(10 * nup + spin)
        mid = sum(1 << k for k in rng.sample(range(1, last), ne - 1))
        other = sum(1 << k for k in rng.sample(range(norb), 8 - ne))
        a, b = mid | 1, mid | (1 << last)
        dets = [(a, other), (b, other)] if spin == 0 else [(other, a), (other, b)]
        c = [0.6, -0.8]
        chk = GC.Greens(HH, dets, c, e0, norb)
        w = [GC.outside(chk.all_poles(), 0.5)[1]]
        out = _check_both(g, chk, dets, c, e0, w, "extremes nup=%d spin=%d" % (nup, spin))
        for p, q in ((0, last), (last, 0)):
            assert chk.count(GC.NM1, p, q) == 1 and chk.count(GC.NP1, p, q) == 1
            e = chk.entry(GC.NM1, p, q, w[0])
            assert out[False][1][0, p, q] / (0.6 * -0.8) > 0.0
            assert e.signed == (-1.0) ** (ne - 1) * e.unsigned and e.signed != 0.0
            assert math.copysign(1.0, out[True][1][0, p, q]) == math.copysign(1.0, e.signed)


def test_diagonals_do_not_depend_on_the_sign_mode(dev):
    h, g, HH = _chem(dev)
    dets = _grown(h, 90)
    c = _normalised(random.Random(90), 90)
    up, dn = _arrays(dets)
    e0 = _e0(HH, h)
    w = [e0 - 9.0, 11.5]
    a, b = g.greens_function(up, dn, c, e0, w, False), g.greens_function(up, dn, c, e0, w, True)
    differ = 0
    for k in (0, 1):
        for p in range(h.norb):
            assert a[k][:, p, p].tobytes() == b[k][:, p, p].tobytes()
        differ += int(np.count_nonzero(a[k] != b[k]))
    assert differ > 20


# ---------------------------------------------------------------------------------------------- 4. spin counts
def _has_equal_strings_intermediate(dets, norb):
    for u, d in dets:
        for q in range(norb):
            if (u ^ (1 << q)) == d or (d ^ (1 << q)) == u:
                return True
    return False


@pytest.mark.parametrize("nelec,nup", [(8, 5), (4, 3), (3, 1), (3, 2)])
def test_spin_counts(dev, nelec, nup):
    """nup != ndn; with nup + 1 = ndn or nup = ndn + 1 an N+-1 determinant can have up == dn (the diagonal's doubling branch): the lists
    of (3, 1) and (3, 2) hold such intermediates; (3, 1) has nup = 1, so its N-1 up part has an empty string.  One output pointer NULL:
    the other half has the bits of the two-output call"""
    h, g, HH = _chem(dev, nelec, nup)
    rng = random.Random(nelec * 10 + nup)
    dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 90)
    if abs(2 * nup - nelec) == 1:
        assert _has_equal_strings_intermediate(dets, h.norb)
    c = _normalised(rng, len(dets))
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, dets, c, e0, h.norb)
    w = GC.outside(chk.all_poles(), 0.5)
    out = _check_both(g, chk, dets, c, e0, w, "nup=%d ndn=%d" % (nup, nelec - nup))
    assert sum(chk.count(GC.NM1, p, q) > 0 for p in range(h.norb) for q in range(h.norb) if p != q) > 20
    up, dn = _arrays(dets)
    only_p = g.greens_function(up, dn, c, e0, w, False, parts="np1")
    only_m = g.greens_function(up, dn, c, e0, w, False, parts="nm1")
    assert only_p[1] is None and only_m[0] is None
    assert only_p[0].tobytes() == out[False][0].tobytes() and only_m[1].tobytes() == out[False][1].tobytes()


# ---------------------------------------------------------------------------------------------- 5. bit 63
def _write_diagonal_fcidump(path, norb, nelec, seed):
    """the records a diagonal element needs and no others: h_pp, (pp|qq) and (pq|qp), seeded; c1"""
    rng = random.Random(seed)
    n = 0
    with open(path, "w") as f:
        f.write(" &FCI NORB=%d,NELEC=%d,MS2=0,\n  ORBSYM=%s,\n  ISYM=1,\n &END\n" % (norb, nelec, ",".join(["1"] * norb)))
        for p in range(1, norb + 1):
            for q in range(1, p + 1):
                f.write("%.17e %d %d %d %d\n" % (rng.uniform(0.2, 0.6), p, p, q, q)); n += 1
                if q < p:
                    f.write("%.17e %d %d %d %d\n" % (rng.uniform(0.01, 0.1), p, q, q, p)); n += 1
        for p in range(1, norb + 1):
            f.write("%.17e %d %d 0 0\n" % (-2.0 + 0.03 * p + rng.uniform(0.0, 0.01), p, p)); n += 1
        f.write("%.17e 0 0 0 0\n" % 1.25)
    return n


def test_bit_63(dev, tmp_path):
    from sqmc_amd import host as H
    path = str(tmp_path / "FCIDUMP_64")
    assert 4000 < _write_diagonal_fcidump(path, 64, 5, 63) < 4400
    h = H.ChemHost(path, 5, 2, "c1")
    assert h.norb == 64
    HH = PC.ChemH(path, [int(h.orb_order[i]) for i in range(1, 65)])
    g = h.gpu()
    try:
        b = lambda *orbs: sum(1 << k for k in orbs)
        dets = [(b(0, 62), b(1, 2, 63)), (b(62, 63), b(1, 2, 63)), (b(0, 62), b(0, 1, 2)), (b(0, 63), b(1, 2, 63)), (b(0, 62), b(0, 1, 63))]
        c = [0.5, -0.4, 0.3, 0.45, -0.35]
        e0 = HH.element(dets[0][0], dets[0][1], dets[0][0], dets[0][1])[0] - 0.05
        chk = GC.Greens(HH, dets, c, e0, 64)
        # creation at bit 63 (up 0 -> 63 through m = {0, 62, 63}), annihilation at bit 63, p = q = 63, the 0 <-> 63 pair of both spins
        assert chk.count(GC.NP1, 0, 63) == 2 and chk.count(GC.NP1, 63, 0) == 2 and chk.count(GC.NM1, 0, 63) == 2 and chk.count(GC.NM1, 63, 0) == 2
        assert chk.count(GC.NM1, 63, 63) == 6 and chk.count(GC.NP1, 63, 63) == 4 and chk.count(GC.NP1, 63, 62) == 1 and chk.count(GC.NM1, 62, 63) == 1
        w = GC.outside(chk.all_poles(), 0.5)
        out = _check_both(g, chk, dets, c, e0, w, "bit 63")
        assert np.all(out[False][0][:, 0, 63] != 0.0) and np.all(out[True][1][:, 63, 0] != 0.0)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 6. order and repeatability
def test_order_and_repeatability(dev):
    h, g, HH = _chem(dev)
    n = 300
    dets = _grown(h, n)
    rng = random.Random(300)
    c = _normalised(rng, n)
    up, dn = _arrays(dets)
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, dets, c, e0, h.norb)
    w = GC.outside(chk.all_poles(), 0.5)
    base = _check_both(g, chk, dets, c, e0, w, "300")[False]
    same = lambda r: r[0].tobytes() == base[0].tobytes() and r[1].tobytes() == base[1].tobytes()
    assert same(g.greens_function(up, dn, c, e0, w))
    cc = np.array(c)
    for order in (sorted(range(n), key=lambda k: dets[k]), list(range(n))[::-1], rng.sample(range(n), n)):
        assert same(g.greens_function(up[order], dn[order], cc[order], e0, w))
    # a zero coefficient: the list without that determinant
    last = max(range(n), key=lambda k: dets[k])                    # sorts last by (up, dn), the order of the ranks
    for k, exact in ((last, True), (n // 2, False)):
        keep = [j for j in range(n) if j != k]
        c0 = cc.copy(); c0[k] = 0.0
        with_zero = g.greens_function(up, dn, c0, e0, w)
        without = g.greens_function(up[keep], dn[keep], cc[keep], e0, w)
        chk0 = GC.Greens(HH, [dets[j] for j in keep], cc[keep].tolist(), e0, h.norb)
        for part, kk in PARTS:
            _compare(chk0, part, False, w, without[kk], "without %d" % k)
            fails, _ = chk0.compare(part, False, w, with_zero[kk])
            assert not fails, fails[:4]
        if exact:
            assert np.array_equal(with_zero[0], without[0]) and np.array_equal(with_zero[1], without[1])


# ---------------------------------------------------------------------------------------------- 7. frequencies
def test_frequency_counts_and_tiling(dev):
    h, g, HH = _chem(dev)
    n = 65
    dets = _grown(h, n)
    c = _normalised(random.Random(65), n)
    up, dn = _arrays(dets)
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, dets, c, e0, h.norb)
    lo, hi = GC.outside(chk.all_poles(), 0.5)
    distinct = [lo, hi, lo - 1.75, hi + 2.5]
    grid = [distinct[(3 * i + i // 7) % 4] for i in range(WTILE + 1)]                      # 257 points: outside points, repeated
    assert len(set(grid)) == 4 and len(grid) == 257
    one = {wv: g.greens_function(up, dn, c, e0, [wv]) for wv in distinct}
    for wv in distinct[:2]:
        for part, k in PARTS:
            _compare(chk, part, False, [wv], one[wv][k], "n_w = 1")
    two = g.greens_function(up, dn, c, e0, distinct[:2])
    big = g.greens_function(up, dn, c, e0, grid)
    for k in (0, 1):
        assert one[lo][k].shape == (1, h.norb, h.norb) and two[k].shape == (2, h.norb, h.norb) and big[k].shape == (257, h.norb, h.norb)
        for i in (0, 1):
            assert two[k][i].tobytes() == one[distinct[i]][k][0].tobytes()
        for i, wv in enumerate(grid):                                                       # every point, the one behind the tile's edge included
            assert big[k][i].tobytes() == one[wv][k][0].tobytes(), i
    first = [grid.index(wv) for wv in distinct]
    for part, k in PARTS:
        _compare(chk, part, False, distinct, big[k][first], "n_w = 257")


# ---------------------------------------------------------------------------------------------- 8. sum rule
def test_sum_rule_against_the_one_rdm_entry(dev):
    """signed mode far outside the poles: w G_nm1(w, p, q) -> <a+_p a_q> and w G_np1(w, p, q) -> 2 delta_pq sum c^2 - <a+_q a_p>, with the
    density matrix from the library's own 1-RDM entry (one_rdm()[p, r] = <a+_r a_p>)"""
    h, g, HH = _chem(dev)
    dets = _grown(h, 90)
    c = _normalised(random.Random(8), 90)
    up, dn = _arrays(dets)
    e0 = _e0(HH, h)
    chk = GC.Greens(HH, dets, c, e0, h.norb)
    rdm, exp = g.one_rdm(up, dn, c), RC.one_rdm(dets, c, h.norb)
    assert not RC.compare(exp, rdm)[0]
    norm2 = 2.0 * math.fsum(x * x for x in c)
    w = [2.0 ** 40, -2.0 ** 40]
    gp, gm = g.greens_function(up, dn, c, e0, w, True)
    n_off = 0
    for i, wv in enumerate(w):
        for p in range(h.norb):
            for q in range(h.norb):
                assert abs(wv * gm[i, p, q] - rdm[q, p]) <= chk.sum_rule_bound(GC.NM1, p, q, wv) + 2.0 * exp.bound(q, p)
                want = (norm2 if p == q else 0.0) - rdm[p, q]
                assert abs(wv * gp[i, p, q] - want) <= chk.sum_rule_bound(GC.NP1, p, q, wv) + 2.0 * exp.bound(p, q) + 8.0 * GC.U * norm2
                n_off += p != q and rdm[q, p] != 0.0
    assert n_off > 40


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(dev):
    from sqmc_amd import host as H
    h, g, HH = _chem(dev)
    dets = _grown(h, 40)
    c = _normalised(random.Random(40), 40)
    up, dn = _arrays(dets)
    e0 = _e0(HH, h)
    n2 = h.norb * h.norb
    L = g.L
    L.sqmc_gpu_hci_greens_function.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.sqmc_gpu_last_error.restype = C.c_char_p
    marked = [np.full(3 * n2, 7.25), np.full(3 * n2, -3.5)]

    def raw(code, word, u=up, d=dn, cc=c, e=e0, w=(-9.0, 10.0), n_w=None, fermi=0, ctx=g, outs=(0, 1)):
        u, d, cc, w = np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(d, np.uint64), np.ascontiguousarray(cc, np.float64), np.ascontiguousarray(w, np.float64)
        ptr = [marked[k].ctypes.data_as(C.c_void_p) if k in outs else None for k in (0, 1)]
        rc = L.sqmc_gpu_hci_greens_function(ctx.h, len(u), u.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), float(e),
                                            len(w) if n_w is None else n_w, w.ctypes.data_as(C.c_void_p), fermi, ptr[0], ptr[1])
        msg = L.sqmc_gpu_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert np.all(marked[0] == 7.25) and np.all(marked[1] == -3.5)

    raw(BAD_ARG, "twice", np.concatenate((up, up[7:8])), np.concatenate((dn, dn[7:8])), np.concatenate((c, [0.1])))
    wrong = up.copy(); wrong[5] |= np.uint64(1 << 20) if not int(wrong[5]) >> 20 & 1 else np.uint64(1 << 21)
    raw(BAD_ARG, "nup / ndn", wrong)
    beyond = up.copy(); beyond[3] = (int(beyond[3]) & ~(1 << PC._bits(int(beyond[3]))[0])) | (1 << 40)
    raw(BAD_ARG, "nup / ndn", beyond)
    raw(BAD_ARG, "bad argument", n_w=0)
    raw(BAD_ARG, "frequency is not finite", w=(1.0, float("nan")))
    raw(BAD_ARG, "frequency is not finite", w=(float("inf"),))
    raw(BAD_ARG, "e0 is not finite", e=float("nan"))
    raw(BAD_ARG, "both outputs", outs=())
    raw(BAD_ARG, "fermi_sign", fermi=2)
    raw(BAD_ARG, "fermi_sign", fermi=-1)
    ts = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1)
    others = [(ts, "determinant-basis expansion"), (H.HegHost(3, 0.5, 14, 7, 1.49), "chem contexts only"), (H.HubbardHost(4, 4, True, 8, 8), "chem contexts only")]
    for hh, word in others:
        gg = hh.gpu()
        try:
            raw(UNSUPPORTED, word, [hh.hf_up], [hh.hf_dn], [1.0], ctx=gg)
            import sqmc_amd
            with pytest.raises(sqmc_amd.SqmcGpuError) as err:
                gg.greens_function([hh.hf_up], [hh.hf_dn], [1.0], -1.0, [0.5])
            assert err.value.code == UNSUPPORTED
        finally:
            gg.close()
    chk = GC.Greens(HH, dets, c, e0, h.norb)                       # an ordinary call after the refusals
    _check_both(g, chk, dets, c, e0, GC.outside(chk.all_poles(), 0.5), "after refusals")


# ---------------------------------------------------------------------------------------------- 10. host layer
def _ts_wavefunction(h, n, z, seed):
    """n time-symmetrised entries (representatives up <= dn; without up == dn for z = -1, where they vanish), seeded coefficients"""
    rng = random.Random(seed)
    grown = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 4 * n)
    reps = []
    for u, d in grown:
        r = (min(u, d), max(u, d))
        if r not in reps and not (z == -1 and u == d):
            reps.append(r)
    reps = reps[:n]
    assert len(reps) == n and any(u != d for u, d in reps)
    return reps, _normalised(rng, n)


@pytest.mark.parametrize("z", [1, -1])
def test_host_layer_on_a_time_symmetrised_wavefunction(dev, z):
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=z)
    HH = PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)])
    reps, c = _ts_wavefunction(h, 40, z, 40 + z)
    up, dn = _arrays(reps)
    du, dd, dc = H.time_symmetrized_to_dets(up, dn, c, z)
    dets = list(zip(du.tolist(), dd.tolist()))
    assert len(dets) > 40 and abs(math.fsum(x * x for x in dc) - 1.0) < 1e-12
    e0 = HH.element(reps[0][0], reps[0][1], reps[0][0], reps[0][1])[0] - 0.05
    chk = GC.Greens(HH, dets, dc.tolist(), e0, h.norb)
    w = GC.outside(chk.all_poles(), 0.5)
    wts = np.stack((np.array(c), np.zeros(len(c))), axis=1)        # two states: state 1 alone is used
    for signed in (False, True):
        got = H.hci_greens_function(h, up, dn, wts, e0, w, fermi_sign=signed)
        for part, k in PARTS:
            _compare(chk, part, signed, w, got[k], "host layer z = %d" % z)


# ---------------------------------------------------------------------------------------------- 11. deck
def _deck_text(group):
    t = open(DECK).read().replace("1e-3  1e-7      1.e-4   2", "1e-3  1e-4      1.e-4   1")
    assert "1e-3  1e-4      1.e-4   1" in t
    return t + group


@pytest.fixture(scope="module")
def deck_case():
    """the deck's conventions (time_sym, z = 1, hf_symmetry = 1); 30 time-symmetrised entries, the energy their Rayleigh quotient"""
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    HH = PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)])
    reps, c = _ts_wavefunction(h, 30, 1, 30)
    up, dn = _arrays(reps)
    order = H.sort_dets(up, dn)
    up, dn, c = up[order], dn[order], np.array(c)[order]
    du, dd, dc = H.time_symmetrized_to_dets(up, dn, c, 1)
    dets = list(zip(du.tolist(), dd.tolist()))
    e0 = GC.rayleigh_quotient(HH, dets, dc.tolist())
    chk = GC.Greens(HH, dets, dc.tolist(), e0, h.norb)
    w_min, w_max = GC.uniform(chk.all_poles(), 5)
    group = "&greens_function get_greens_function=t n_w=5 w_min=%r w_max=%r /\n" % (w_min, w_max)
    return h, up, dn, c, e0, chk, group


def _run_deck(tmp, case, group, **kw):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    h, up, dn, c, e0, chk, _ = case
    os.makedirs(tmp, exist_ok=True)
    H.write_wf_var(os.path.join(tmp, H.wf_filename(1e-3)), up, dn, c.reshape(-1, 1), np.array([e0]))
    here = os.getcwd()
    os.chdir(tmp)
    try:
        buf = io.StringIO()
        deck = R.parse_hci_deck(_deck_text(group))
        return deck, R.run_hci(deck, FCIDUMP, out=buf, **kw), buf.getvalue().splitlines()
    finally:
        os.chdir(here)


def _check_files(tmp, chk, w, signed):
    from sqmc_amd import host as H
    norb = chk.norb
    for name, part in (("G0_N+1", GC.NP1), ("G0_N-1", GC.NM1)):
        header, rec = H.read_greens_function(os.path.join(tmp, name))
        assert header == H.GREENS_HEADERS[name]
        where = {wv: i for i, wv in enumerate(w.tolist())}
        keys = [(where[r[0]], r[2], r[1]) for r in rec]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)         # i_w, then q, then p
        seen = {(where[r[0]], r[1] - 1, r[2] - 1): r[3] for r in rec}
        for i, wv in enumerate(w.tolist()):
            for p in range(norb):
                for q in range(norb):
                    e = chk.entry(part, p, q, wv)
                    if e.n:
                        assert e.bound < GC.REL_BOUND_MAX * e.sum_abs
                    if (i, p, q) in seen:
                        v = seen[(i, p, q)]
                        assert abs(v) > 1e-8 and abs(v - e.value(signed)) <= e.bound, (name, i, p, q)
                    else:
                        assert abs(e.value(signed)) <= 1e-8 + e.bound, (name, i, p, q)
        assert len(rec) > 100
    header, rho = H.read_greens_function(os.path.join(tmp, "rho"))
    assert header == H.GREENS_HEADERS["rho"] and rho.shape == (5, 4) and np.array_equal(rho[:, 0], w)
    assert np.array_equal(rho[:, 3], rho[:, 1] + rho[:, 2])
    return rho


def test_deck(dev, deck_case, tmp_path):
    from sqmc_amd import host as H
    h, up, dn, c, e0, chk, group = deck_case
    tmp = str(tmp_path / "plain")
    deck, res, lines = _run_deck(tmp, deck_case, group)
    assert deck["get_greens_function"] and deck["n_w"] == 5
    w, gp, gm = res["greens"]
    assert np.array_equal(w, H.greens_grid(5, deck["w_min"], deck["w_max"]))
    rho = _check_files(tmp, chk, w, False)
    assert np.array_equal(rho[:, 1:], H.density_of_states(gp, gm))
    at = [k for k, l in enumerate(lines) if l.startswith(" About to compute Green's function for           5 frequencies:")]
    assert len(at) == 1 and lines[at[0] + 1] == "".join(H._es24(x) for x in w) and lines[at[0] + 2] == " E_0 =" + H._es24(e0)
    pt = [k for k, l in enumerate(lines) if l.startswith("2nd-order PT energy lowering(1)=") or l.startswith("Total energy(1)=")]
    assert len(pt) == 2 and pt[0] > at[0] and len(res["states"]) == 1
    # a second run in the same directory stops on the existing files, before anything else
    with pytest.raises(FileExistsError):
        _run_deck(tmp, deck_case, group)
    # --greens-signed: the checker's signed values; rho unchanged
    tmp_s = str(tmp_path / "signed")
    _, res_s, _ = _run_deck(tmp_s, deck_case, group, greens_signed=True)
    rho_s = _check_files(tmp_s, chk, w, True)
    assert rho_s.tobytes() == rho.tobytes()
    flipped = sum(1 for p in range(h.norb) for q in range(h.norb) if p != q and res_s["greens"][2][0, p, q] == -gm[0, p, q] != 0.0)
    assert flipped > 10
    # the same deck without the group: no file, the PT lines as before
    tmp_n = str(tmp_path / "none")
    _, res_n, lines_n = _run_deck(tmp_n, deck_case, "")
    assert "greens" not in res_n and not any(os.path.exists(os.path.join(tmp_n, f)) for f in H.GREENS_HEADERS)
    assert res_n["states"] == res["states"] and not any("Green" in l for l in lines_n)
