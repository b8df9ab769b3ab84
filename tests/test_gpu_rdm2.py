"""The 2-RDM entry of the HIP library (sqmc_gpu_hci_2rdm), GpuChem.two_rdm, the host layer around it and the --two-rdm stage of the deck
runner against tests/rdm2_checker.py, which shares nothing with the library.  Every comparison bound of an entry is the checker's
derived rounding bound; exact zeros, symmetries and reproducibility are compared with == or on the bytes.  The Gram kernel gives an
entry to a wavefront (64 lanes) or a block (256 threads) and the record sort works on tiles of 1024: the list sizes straddle them."""
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
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402
from tests import rdm2_checker as R2         # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
OK, BAD_ARG, ERR_HIP, UNSUPPORTED = 0, -1, -2, -3
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
SAMPLED = SIZES[-3:]
V = C.c_void_p


def _arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


def _normalised(rng, n, zeros=True):
    """random, normalised, and every seventh coefficient an exact zero (lists of three and more)"""
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    if zeros and n >= 3:
        for k in range(1, n, 7):
            c[k] = 0.0
    s = math.sqrt(math.fsum(x * x for x in c))
    return [x / s for x in c]


def _neighbours(rng, start, norb, n):
    """n distinct determinants grown from start by single-orbital moves of members"""
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


_CHEM, _SD = {}, {}


def _chem(dev, nelec=8, nup=4):
    from sqmc_amd import host as H
    key = (nelec, nup)
    if key not in _CHEM:
        h = H.ChemHost(FCIDUMP, nelec, nup, "d2h")
        _CHEM[key] = (h, h.gpu(), PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)]))
    return _CHEM[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for _, g, _ in _CHEM.values():
        g.close()
    _CHEM.clear(); _CASE.clear()


def _sd_list(h, rng, n):
    """HF, up to 16 of its single excitations and random doubles: n determinants in random order"""
    if "u" not in _SD:
        hf = (int(h.hf_up), int(h.hf_dn))
        _SD["u"] = sorted(set((int(a), int(b)) for a, b in PC.excitations_chem(hf[0], hf[1], h.norb)) - {hf})
        _SD["singles"] = [d for d in _SD["u"] if PC._pop(d[0] ^ hf[0]) + PC._pop(d[1] ^ hf[1]) == 2]
    lst = [(int(h.hf_up), int(h.hf_dn))] + rng.sample(_SD["singles"], min(16, max(n - 1, 0)))
    pool = [d for d in _SD["u"] if d not in set(lst)]
    lst += rng.sample(pool, n - len(lst))
    rng.shuffle(lst)
    return lst[:n]


def _mask(reached, norb):
    m = np.zeros((norb,) * 4, bool)
    if reached:
        m[tuple(np.array(sorted(reached)).T)] = True
    return m


class _Every8th:
    """a fixed seeded sample of the norb^4 entries of a block"""

    def __init__(self, seed):
        self.seed = seed

    def __contains__(self, idx):
        return (7 * idx[0] + 11 * idx[1] + 13 * idx[2] + 17 * idx[3] + self.seed) % 8 == 0


def _check(g, dets, c, norb, tag="", sampled=False, seed=0, blocks="all"):
    """the device's blocks of a list against the checker: every entry, or (sampled) a few thousand seeded entries with terms plus the
    whole-array zero pattern from the entries the checker's pass reaches"""
    up, dn = _arrays(dets)
    got = g.two_rdm(up, dn, c, blocks)
    names = tuple(got)
    if sampled:                                  # one pass of the checker: the terms of every 8th entry, and the set of all reached ones
        exp = R2.two_rdm(dets, c, norb, {b: _Every8th(seed) for b in R2.BLOCKS})
        sample = {b: set(exp.terms[b]) for b in R2.BLOCKS}
        assert 3000 <= sum(len(sample[b]) for b in R2.BLOCKS) <= 30000, {b: len(sample[b]) for b in R2.BLOCKS}
    else:
        sample, exp = None, R2.two_rdm(dets, c, norb)
    fails, worst, seen = R2.compare(exp, got, names, sample)
    print("%s n = %d: %d entries compared, worst |delta| / bound = %.3f" % (tag, len(dets), seen, worst))
    assert not fails, fails[:4]
    for b in names:                              # every entry no pair of determinants reaches is exactly 0.0
        assert np.count_nonzero(got[b][~_mask(exp.reached[b], norb)]) == 0, b
    return got, exp


# ---------------------------------------------------------------------------------------------- 1. entries against the checker
@pytest.mark.parametrize("kind", ["sd", "neighbours"])
@pytest.mark.parametrize("n", SIZES)
def test_entries_chem(dev, n, kind):
    """C2, (nelec, nup) = (8, 4), 26 orbitals: HF + singles + doubles, and lists grown by single moves"""
    h, g, _ = _chem(dev)
    rng = random.Random(2000 + n + (0 if kind == "sd" else 50000))
    dets = _sd_list(h, rng, n) if kind == "sd" else _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, n)
    c = _normalised(rng, n)
    got, exp = _check(g, dets, c, h.norb, tag=kind, sampled=n in SAMPLED, seed=n)
    n2 = R2.norm2(c)
    for b, want in (("aa", 12), ("bb", 12), ("ab", 16)):
        tr = math.fsum(float(got[b][p, q, p, q]) for p in range(h.norb) for q in range(h.norb))
        assert abs(tr - want * n2) <= PC.rounding_bound(n, want * n2) + 26 * 26 * RC.U * want * n2, (b, tr)


# ---------------------------------------------------------------------------------------------- 2. electron-count edges
@pytest.mark.parametrize("nup,ndn", [(1, 3), (3, 0), (1, 1), (3, 1)])
def test_electron_count_edges(dev, nup, ndn):
    from sqmc_amd import host as H
    h = H.HubbardHost(4, 4, True, nup, ndn)
    g = h.gpu()
    try:
        rng = random.Random(10 * nup + ndn)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 70)
        c = _normalised(rng, len(dets))
        got, exp = _check(g, dets, c, h.norb, tag="nup=%d ndn=%d" % (nup, ndn))
        for b, live in (("aa", nup >= 2), ("bb", ndn >= 2), ("ab", nup >= 1 and ndn >= 1)):
            assert (np.count_nonzero(got[b]) > 0) == live, b
            assert live or (not np.any(np.signbit(got[b])) and got[b].shape == (16,) * 4)
    finally:
        g.close()


def test_chem_with_one_dn_electron(dev):
    h, g, _ = _chem(dev, 4, 3)
    rng = random.Random(43)
    dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 90)
    got, _ = _check(g, dets, _normalised(rng, len(dets)), h.norb, tag="chem nup=3 ndn=1")
    assert np.count_nonzero(got["bb"]) == 0 and np.count_nonzero(got["aa"]) > 100 and np.count_nonzero(got["ab"]) > 100


def test_single_determinant(dev):
    h, g, _ = _chem(dev)
    c = 0.75
    got = g.two_rdm([h.hf_up], [h.hf_dn], [c])
    ou, od = RC.occupation(int(h.hf_up)), RC.occupation(int(h.hf_dn))
    for b, left, right in (("aa", ou, ou), ("bb", od, od), ("ab", ou, od)):
        want = np.zeros((h.norb,) * 4)
        for p in left:
            for q in right:
                if b == "ab" or p != q:
                    want[p, q, p, q] = c * c
                    if b != "ab":
                        want[p, q, q, p] = -(c * c)
        assert np.array_equal(got[b], want), b


# ---------------------------------------------------------------------------------------------- 3. bits 0 and 63
def test_bits_0_and_63_on_the_8x8_lattice(dev):
    from sqmc_amd import host as H
    h = H.HubbardHost(8, 8, True, 3, 2)
    g = h.gpu()
    try:
        a_up, dn0 = (1 << 0) | (1 << 5) | (1 << 9), (1 << 62) | (1 << 3)
        dets = [(a_up, dn0), ((a_up ^ 1) | (1 << 63), dn0), (a_up, (1 << 63) | (1 << 3)), (a_up, (1 << 63) | (1 << 0)),
                ((1 << 62) | (1 << 5) | (1 << 9), dn0), ((1 << 63) | (1 << 62) | (1 << 61), dn0), ((1 << 63) | (1 << 5) | (1 << 0), (1 << 63) | (1 << 0))]
        c = [0.5, -0.4, 0.3, 0.45, -0.35, 0.4, 0.25]
        up, dn = _arrays(dets)
        exp = R2.two_rdm(dets, c, 64)
        for b in R2.BLOCKS:                                          # one block per call: 134 MB each
            got = g.two_rdm(up, dn, c, b)
            assert list(got) == [b]
            a = got[b]
            for idx in exp.terms[b]:
                x, want, bd = float(a[idx]), exp.value(b, idx), exp.bound(b, idx)
                assert abs(x - want) <= bd, (b, idx, x, want)
            live = sum(1 for idx in exp.terms[b] if exp.value(b, idx) != 0.0)
            assert np.count_nonzero(a) == live and live > 20, (b, live)
            if b == "ab":
                assert exp.count("ab", (63, 63, 63, 63)) == 1 and a[63, 63, 63, 63] == 0.25 * 0.25 and a[0, 0, 0, 0] == 0.45 * 0.45 + 0.25 * 0.25
            del got, a
    finally:
        g.close()


def test_two_pass_order_on_the_8x8_lattice(dev):
    """8 up and 7 dn electrons on 64 sites: the intermediates of every block need 55 or 56 key bits, which with the 11 or 12 bits of
    the pair index pass one word, so the records are ordered by two stable sorts (K, then the pair)"""
    from sqmc_amd import host as H
    h = H.HubbardHost(8, 8, True, 8, 7)
    g = h.gpu()
    try:
        rng = random.Random(87)
        start = (int(h.hf_up) | (1 << 63) | 1, int(h.hf_dn) | (1 << 63) | 1)
        while bin(start[0]).count("1") > 8:
            start = (start[0] & ~(1 << RC.occupation(start[0])[1]), start[1])
        while bin(start[1]).count("1") > 7:
            start = (start[0], start[1] & ~(1 << RC.occupation(start[1])[1]))
        dets = _neighbours(rng, start, 64, 40)
        c = _normalised(rng, len(dets))
        up, dn = _arrays(dets)
        exp = R2.two_rdm(dets, c, 64)
        for b in R2.BLOCKS:
            a = g.two_rdm(up, dn, c, b)[b]
            worst = 0.0
            for idx in exp.terms[b]:
                x, want, bd = float(a[idx]), exp.value(b, idx), exp.bound(b, idx)
                assert abs(x - want) <= bd, (b, idx, x, want)
                worst = max(worst, abs(x - want) / bd if bd else 0.0)
            live = sum(1 for idx in exp.terms[b] if exp.value(b, idx) != 0.0)
            print("two passes, %s: %d entries with terms, worst |delta| / bound = %.3f" % (b, len(exp.terms[b]), worst))
            assert np.count_nonzero(a) == live and live > 200, (b, live)
            assert a.tobytes(order="F") == g.two_rdm(up[::-1], dn[::-1], c[::-1], b)[b].tobytes(order="F")
            del a
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 4, 5. symmetries and reproducible bytes
_CASE = {}


def _case(dev, n=300):
    """one list of the C2 fixture with its device blocks and 1-RDM, its checker matrices and <H>, shared by the tests below"""
    if n not in _CASE:
        h, g, HH = _chem(dev)
        rng = random.Random(4242 + n)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, n // 2) if n > 100 else []
        dets = dets + [d for d in _sd_list(h, rng, n) if d not in set(dets)][:n - len(dets)]
        c = _normalised(rng, len(dets))
        up, dn = _arrays(dets)
        _CASE[n] = dict(dets=dets, c=c, up=up, dn=dn, got=g.two_rdm(up, dn, c), one=g.one_rdm(up, dn, c))
    return _CASE[n]


def test_exact_symmetries(dev):
    got = _case(dev)["got"]
    norb = got["aa"].shape[0]
    for b in R2.BLOCKS:
        assert np.count_nonzero(got[b]) > 1000
        assert np.array_equal(got[b], got[b].transpose(2, 3, 0, 1)), b
    for b in ("aa", "bb"):
        assert np.array_equal(got[b], -got[b].transpose(1, 0, 2, 3)) and np.array_equal(got[b], -got[b].transpose(0, 1, 3, 2)), b
        assert np.array_equal(got[b], got[b].transpose(1, 0, 3, 2))
        for p in range(norb):
            assert np.count_nonzero(got[b][p, p]) == 0 and np.count_nonzero(got[b][:, :, p, p]) == 0
        assert not np.any(np.signbit(got[b][got[b] == 0.0]))          # no -0.0 among the images


def test_same_bits_again_shuffled_and_alone(dev):
    h, g, _ = _chem(dev)
    cs = _case(dev)
    up, dn, c, got = cs["up"], cs["dn"], np.array(cs["c"]), cs["got"]
    again = g.two_rdm(up, dn, c)
    order = np.random.RandomState(5).permutation(len(c))
    shuffled = g.two_rdm(up[order], dn[order], c[order])
    for b in R2.BLOCKS:
        assert again[b].tobytes(order="F") == got[b].tobytes(order="F") == shuffled[b].tobytes(order="F"), b
        alone = g.two_rdm(up, dn, c, b)
        assert list(alone) == [b] and alone[b].tobytes(order="F") == got[b].tobytes(order="F"), b
    two = g.two_rdm(up, dn, c, ("aa", "ab"))
    assert sorted(two) == ["aa", "ab"] and all(two[b].tobytes(order="F") == got[b].tobytes(order="F") for b in two)


def test_heavy_columns_take_the_block_owner(dev):
    """1050 determinants, two up strings {0,1,2,3} and {0,1,2,4} times 525 random dn strings: the aa columns of the pairs inside them
    hold 1050 or 525 records, past the 512 at which an entry goes to a 256-thread block.  G_aa[2,3,2,4] then has 525 terms, the
    diagonal ones 1050; the ab and bb columns stay short.  Sampled entries and the zero pattern against the checker, the bytes twice"""
    h, g, _ = _chem(dev)
    rng = random.Random(8)
    dns = set()
    while len(dns) < 525:
        dns.add(sum(1 << k for k in rng.sample(range(h.norb), 4)))
    dets = [(u, d) for u in (0b01111, 0b10111) for d in sorted(dns)]
    rng.shuffle(dets)
    c = _normalised(rng, len(dets))
    up, dn = _arrays(dets)
    got = g.two_rdm(up, dn, c)
    five = [(p, q, r, s) for p in range(5) for q in range(5) for r in range(5) for s in range(5)]
    sample = {"aa": set(five), "bb": set(five) | {tuple(rng.randrange(26) for _ in range(4)) for _ in range(300)},
              "ab": {(p, rng.randrange(26), r, rng.randrange(26)) for p in range(5) for r in range(5) for _ in range(40)}}
    exp = R2.two_rdm(dets, c, h.norb, sample)
    fails, worst, seen = R2.compare(exp, got, R2.BLOCKS, sample)
    print("heavy: %d entries compared, worst |delta| / bound = %.3f" % (seen, worst))
    assert not fails, fails[:4]
    assert exp.count("aa", (2, 3, 2, 4)) == 525 and exp.count("aa", (0, 1, 0, 1)) == 1050 and exp.count("aa", (0, 3, 0, 3)) == 525
    assert got["aa"][2, 3, 2, 4] != 0.0 and sum(exp.count("ab", k) > 0 for k in sample["ab"]) > 50
    for b in R2.BLOCKS:
        assert np.count_nonzero(got[b][~_mask(exp.reached[b], h.norb)]) == 0
    again = g.two_rdm(up, dn, c)
    assert all(again[b].tobytes(order="F") == got[b].tobytes(order="F") for b in R2.BLOCKS)


# ---------------------------------------------------------------------------------------------- 6. identities on the device's output
def _device_energy(HH, one, d, n2):
    """(E, sum |term|) from the device's matrices with the checker's integrals, summed with fsum"""
    vals = [HH.const * n2]
    for p, r in np.argwhere(one != 0.0).tolist():
        vals.append(HH.t(p, r) * float(one[p, r]))
    for b in R2.BLOCKS:
        w = 1.0 if b == "ab" else 0.5
        for p, q, r, s in np.argwhere(d[b] != 0.0).tolist():
            vals.append(w * HH.v(p, r, q, s) * float(d[b][p, q, r, s]))
    return math.fsum(vals), math.fsum(abs(x) for x in vals)


def test_identities_chem(dev):
    from sqmc_amd import host as H
    import sqmc_amd
    h, g, HH = _chem(dev)
    cs = _case(dev, 120)
    dets, c, got, one = cs["dets"], cs["c"], cs["got"], cs["one"]
    norb, n, n2 = h.norb, len(dets), R2.norm2(cs["c"])
    exp2, exp1 = R2.two_rdm(dets, c, norb), RC.one_rdm(dets, c, norb)
    assert not R2.compare(exp2, got)[0] and not RC.compare(exp1, one)[0]
    sf = H.spin_free_two_rdm(got)
    # partial trace = (N - 1) times the device's own 1-RDM (one[p, r] = <a+_r a_p>)
    worst = 0.0
    for p in range(norb):
        for r in range(norb):
            want, bw = R2.partial_trace(exp2, p, r, 8)
            x = math.fsum(float(sf[p, q, r, q]) for q in range(norb))
            bound = 2 * bw + 7 * exp1.bound(r, p) + 8 * RC.U * abs(want)
            assert abs(x - 7 * float(one[r, p])) <= bound, (p, r, x, 7 * one[r, p], bound)
            worst = max(worst, abs(x - 7 * float(one[r, p])) / bound if bound else 0.0)
    # energy: the device's matrices with the checker's integrals against the checker's <Psi|H|Psi>
    e_chk, b_chk = R2.energy(HH, exp1, exp2, n2)
    want, bw, sa = R2.expectation(HH, dets, c)
    e_dev, sa_dev = _device_energy(HH, one, got, n2)
    print("identities: partial trace worst %.3f of its bound; E(device matrices) = %.12f, <H> = %.12f, |delta| = %.3g, bound = %.3g"
          % (worst, e_dev, want, abs(e_dev - want), 2 * b_chk + bw))
    assert abs(e_dev - want) <= 2 * b_chk + bw
    assert abs(e_chk - want) <= b_chk + bw
    # host.rdm_energy: the library's own integrals and numpy's sums over all norb^4 entries
    e_host = H.rdm_energy(h, one, sf)
    assert abs(e_host - want) <= 2 * b_chk + bw + (norb ** 4) * RC.U * sa_dev
    # c . (H c) from the library's resident plan of the same list: pins the sign convention to h_any
    order = H.sort_dets(cs["up"], cs["dn"])
    plan, _, _ = sqmc_amd.SpmvPlan.from_dets(g, cs["up"][order], cs["dn"][order])
    try:
        cv = np.array(c)[order]
        e_plan = float(np.dot(cv, plan.apply(cv)))
    finally:
        plan.close()
    print("c.Hc = %.12f, |E(device matrices) - c.Hc| = %.3g" % (e_plan, abs(e_dev - e_plan)))
    assert abs(e_plan - want) <= bw + 4 * n * RC.U * sa
    assert abs(e_dev - e_plan) <= 2 * b_chk + 2 * bw + 4 * n * RC.U * sa
    # <S^2>
    s_dev = (0.0 + 0.0 + 4) * n2 - math.fsum(float(got["ab"][q, p, p, q]) for p in range(norb) for q in range(norb))
    s_chk = R2.s_squared(dets, c, norb)
    bs = math.fsum(exp2.bound("ab", (q, p, p, q)) for p in range(norb) for q in range(norb)) + (norb * norb + n) * RC.U * (4 * n2 + 16 * n2)
    assert abs(s_dev - s_chk) <= bs, (s_dev, s_chk, bs)
    assert abs(H.s_squared(h, got["ab"], n2) - s_chk) <= 2 * bs
    assert s_chk > 0.01                                   # random coefficients: not a spin eigenstate


def test_identities_hubbard(dev):
    """4 x 4 periodic lattice: U sum_i G_ab[i,i,i,i] - t sum over bonds of D against the plan's c . H c"""
    from sqmc_amd import host as H
    import sqmc_amd
    t, U = 1.0, 4.0
    h = H.HubbardHost(4, 4, True, 3, 3, t, U)
    HH = PC.HubbardH(4, 4, True, t, U)
    g = h.gpu()
    try:
        rng = random.Random(16)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), 16, 150)
        c = _normalised(rng, len(dets))
        up, dn = _arrays(dets)
        got, exp2 = _check(g, dets, c, 16, tag="hubbard 4x4")
        one, exp1 = g.one_rdm(up, dn, c), RC.one_rdm(dets, c, 16)
        inter = [U * float(got["ab"][i, i, i, i]) for i in range(16)]
        hop = [-t * (float(one[i, j]) + float(one[j, i])) for i, j in HH.bonds]
        e_dev = math.fsum(inter + hop)
        bound = U * math.fsum(exp2.bound("ab", (i, i, i, i)) for i in range(16)) + t * math.fsum(exp1.bound(i, j) + exp1.bound(j, i) for i, j in HH.bonds)
        bound += 64 * RC.U * math.fsum(abs(x) for x in inter + hop)
        want, bw, sa = R2.expectation(HH, dets, c)
        assert abs(e_dev - want) <= bound + bw, (e_dev, want, bound + bw)
        order = H.sort_dets(up, dn)
        plan, _, _ = sqmc_amd.SpmvPlan.from_dets(g, up[order], dn[order])
        try:
            cv = np.array(c)[order]
            e_plan = float(np.dot(cv, plan.apply(cv)))
        finally:
            plan.close()
        print("hubbard: U sum G_ab - t sum D = %.12f, c.Hc = %.12f, <H> = %.12f" % (e_dev, e_plan, want))
        assert abs(e_dev - e_plan) <= bound + 2 * bw + 4 * len(c) * RC.U * sa
        assert abs(H.rdm_energy(h, one, H.spin_free_two_rdm(got)) - want) <= bound + bw + 16 ** 4 * RC.U * sa
        assert abs(math.fsum(inter)) > 1e-3
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def _raw(L, ctx, u, d, cc, blocks, outs):
    u, d, cc = np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(d, np.uint64), np.ascontiguousarray(cc, np.float64)
    L.sqmc_gpu_hci_2rdm.argtypes = [V, C.c_int64, V, V, V, C.c_int32, V, V, V]
    return L.sqmc_gpu_hci_2rdm(ctx.h, len(u), u.ctypes.data_as(V), d.ctypes.data_as(V), cc.ctypes.data_as(V), blocks,
                               *[None if a is None else a.ctypes.data_as(V) for a in outs])


def test_refusals_leave_the_outputs_untouched(dev):
    from sqmc_amd import host as H
    h, g, _ = _chem(dev)
    L = g.L
    rng = random.Random(77)
    dets = _sd_list(h, rng, 100)
    c = _normalised(rng, 100)
    up, dn = _arrays(dets)
    outs = [np.full(h.norb ** 4, 7.25) for _ in range(3)]
    untouched = lambda: all(bool(np.all(a == 7.25)) for a in outs)
    twice = np.concatenate((up, up[41:42])), np.concatenate((dn, dn[41:42])), np.concatenate((c, [0.1]))
    assert _raw(L, g, *twice, 7, outs) == BAD_ARG and untouched()
    wrong = up.copy(); wrong[5] |= np.uint64(1 << 20) if not int(wrong[5]) >> 20 & 1 else np.uint64(1 << 21)
    assert _raw(L, g, wrong, dn, c, 7, outs) == BAD_ARG and untouched()
    beyond = up.copy(); beyond[3] = (int(beyond[3]) & ~(1 << PC._bits(int(beyond[3]))[0])) | (1 << 40)
    assert _raw(L, g, beyond, dn, c, 7, outs) == BAD_ARG and untouched()
    for blocks in (0, 8, -1):
        assert _raw(L, g, up, dn, c, blocks, outs) == BAD_ARG and untouched()
    for k in range(3):
        holes = [None if j == k else outs[j] for j in range(3)]
        assert _raw(L, g, up, dn, c, 7, holes) == BAD_ARG and untouched()
        assert _raw(L, g, up, dn, c, 1 << k, holes) == BAD_ARG and untouched()
    assert _raw(L, g, up[:0], dn[:0], c[:0], 7, outs) == BAD_ARG and untouched()
    ts = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1)
    gt = ts.gpu()
    try:
        assert _raw(L, gt, up, dn, c, 7, outs) == UNSUPPORTED and untouched()
        with pytest.raises(dev.SqmcGpuError) as e:
            gt.two_rdm(up, dn, c)
        assert e.value.code == UNSUPPORTED
    finally:
        gt.close()
    hk = H.HubbardKHost(4, 4, 2, 2, 1.0, 4.0, space_sym=True, z=1, p=1, start=(17, 3))
    gk = hk.gpu()
    try:
        small = [np.full(16 ** 4, 7.25) for _ in range(3)]
        assert _raw(L, gk, [hk.hf_up], [hk.hf_dn], [1.0], 7, small) == UNSUPPORTED and all(bool(np.all(a == 7.25)) for a in small)
    finally:
        gk.close()
    with pytest.raises(ValueError):
        g.two_rdm(up, dn, c, "ba")
    # a good call afterwards, with a block left out and its pointer null
    assert _raw(L, g, up, dn, c, 5, [outs[0], None, outs[2]]) == OK and bool(np.all(outs[1] == 7.25))
    ref = g.two_rdm(up, dn, c)
    assert outs[0].tobytes() == ref["aa"].tobytes(order="F") and outs[2].tobytes() == ref["ab"].tobytes(order="F")


# ---------------------------------------------------------------------------------------------- 8. scratch
def test_every_take_fails_in_turn(dev):
    h, g, _ = _chem(dev)
    L = g.L
    L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]
    L.sqmc_gpu_debug_scratch_fail_at.argtypes = [C.c_int64]

    def counters():
        a = [C.c_int64() for _ in range(4)]
        assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 0) == OK
        return tuple(x.value for x in a)
    rng = random.Random(3)
    dets = _sd_list(h, rng, 40)
    c = _normalised(rng, 40)
    up, dn = _arrays(dets)
    outs = [np.full(h.norb ** 4, 7.25) for _ in range(3)]
    base = counters()
    assert _raw(L, g, up, dn, c, 7, outs) == OK
    first = [a.copy() for a in outs]
    after = counters()
    assert after[:2] == base[:2]
    takes = after[3] - base[3]
    assert 20 <= takes <= 200, takes
    for a in outs:
        a[:] = 7.25
    for k in range(1, takes + 1):
        assert L.sqmc_gpu_debug_scratch_fail_at(k) == OK
        rc = _raw(L, g, up, dn, c, 7, outs)
        L.sqmc_gpu_debug_scratch_fail_at(0)
        assert rc == ERR_HIP, (k, takes, rc, L.sqmc_gpu_last_error())
        assert counters()[:2] == base[:2], (k, "live allocations after a failed take")
        assert all(bool(np.all(a == 7.25)) for a in outs), (k, "a failed call wrote an output")
    assert _raw(L, g, up, dn, c, 7, outs) == OK
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, first)) and counters()[:2] == base[:2]
    print("2-RDM: %d takes, every early return balanced" % takes)


# ---------------------------------------------------------------------------------------------- 9. host layer and deck
@pytest.fixture(scope="module")
def ts_wavefunction(dev):
    """i_1sigma_g conventions, two states, one iteration at eps_var 5e-3: a few hundred time-symmetrised determinants, and the
    residual norms |H w - E w| of the two states from a plan in the symmetrised basis"""
    from sqmc_amd import host as H
    import sqmc_amd
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    g = h.gpu()
    try:
        g.set_hb_tables(*h.hb_tables(g))
        up, dn, w, e, hist = H.hci_variational(h, g, 5e-3, n_states=2, max_iters=1)
        order = H.sort_dets(up, dn)
        plan, _, _ = sqmc_amd.SpmvPlan.from_dets(g, up[order], dn[order])
        try:
            res = [float(np.linalg.norm(plan.apply(w[order, i]) - e[i] * w[order, i])) for i in range(2)]
        finally:
            plan.close()
    finally:
        g.close()
    assert 50 <= len(up) <= 1500, hist
    return h, up, dn, w, e, res


def test_host_layer_on_a_time_symmetrised_wavefunction(ts_wavefunction):
    from sqmc_amd import host as H
    h, up, dn, w, e, res = ts_wavefunction
    HH = PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)])
    d0, d1, both = H.hci_two_rdm(h, up, dn, w[:, 0]), H.hci_two_rdm(h, up, dn, w[:, 1]), H.hci_two_rdm(h, up, dn, w)
    for b in R2.BLOCKS:
        assert np.array_equal(both[b], (d0[b] + d1[b]) / 2), b
    du, dd, dc = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
    dets, c = list(zip(du.tolist(), dd.tolist())), dc.tolist()
    exp2, exp1 = R2.two_rdm(dets, c, h.norb), RC.one_rdm(dets, c, h.norb)
    fails, worst, seen = R2.compare(exp2, d0)
    print("host layer: %d combinations, %d determinants, %d entries, worst |delta| / bound = %.3f" % (len(up), len(dets), seen, worst))
    assert not fails, fails[:4]
    n2 = R2.norm2(c)
    _, b_chk = R2.energy(HH, exp1, exp2, n2)
    sf = H.spin_free_two_rdm(d0)
    one = np.einsum("pqrq->rp", sf) / 7.0
    e_dev, sa = _device_energy(HH, one, d0, n2)
    # one is formed from the device's entries here: norb more additions per entry of the one-body part
    bound = 2 * b_chk + (h.norb ** 4 + 64) * RC.U * sa + res[0] * math.sqrt(n2) + abs(e[0]) * abs(n2 - 1.0)
    print("E(matrices) = %.12f, Davidson E_var = %.12f, |delta| = %.3g, bound = %.3g (residual %.3g)" % (e_dev, e[0], abs(e_dev - e[0]), bound, res[0]))
    assert abs(e_dev - e[0]) <= bound
    assert abs(H.rdm_energy(h, one, sf) - e[0]) <= bound
    s2 = H.s_squared(h, d0["ab"], n2)
    # numpy adds the norb^2 exchange entries in its own order: norb^2 more roundings on their mass
    assert abs(s2 - R2.s_squared(dets, c, h.norb)) <= R2.s_squared_bound(dets, c, h.norb, exp2) + h.norb ** 2 * RC.U * float(np.abs(np.einsum("qppq->qp", d0["ab"])).sum())


def _deck_text():
    t = open(DECK).read().replace("1e-3  1e-7", "5e-3  1e-5").replace("eps_var_sched=2*2e-3", "eps_var_sched=2*1e-2")
    assert "5e-3  1e-5" in t and "2*1e-2" in t
    return t


def test_deck_with_two_rdm(dev, tmp_path):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    deck = R.parse_hci_deck(_deck_text())
    buf, path = io.StringIO(), str(tmp_path / "two_rdm.npz")
    res = R.run_hci(deck, FCIDUMP, out=buf, two_rdm_path=path)
    lines = buf.getvalue().splitlines()
    marks = ["Computing 2-RDM of the variational wavefunction in spin blocks aa, bb, ab", "2-RDM of state   1:", "2-RDM of state   2:",
             "2-RDM blocks written to " + path, "State   1:", "State   2:"]
    at = [lines.index(m) for m in marks]
    assert at == sorted(at) and len(set(at)) == len(at)
    i0 = lines.index("2-RDM of state   1:")
    assert lines[i0 + 1].startswith(" sum c^2 =") and abs(float(lines[i0 + 1].split("=")[1]) - 1.0) < 1e-9
    for k, (b, want) in enumerate((("aa", 6), ("bb", 6), ("ab", 16))):
        t = lines[i0 + 2 + k].split()
        assert t[:2] == ["trace", b] and abs(float(t[3]) - want) < 1e-8 and int(t[-1]) == want, lines[i0 + 2 + k]
    t = lines[i0 + 5]
    assert t.startswith(" Energy from the density matrices =") and abs(float(t.split("difference =")[1])) < 1e-6
    assert lines[i0 + 6].startswith(" <S^2> =")
    assert abs(res["two_rdm"][0]["energy"] - res["states"][0][0]) < 1e-6 and abs(res["two_rdm"][1]["energy"] - res["states"][1][0]) < 1e-6
    z = np.load(path)
    assert sorted(z.files) == ["aa_1", "aa_2", "ab_1", "ab_2", "bb_1", "bb_2"] and z["ab_2"].shape == (26,) * 4
    # the same deck without the flag: exactly the lines of before (all but the last, which reports wall-clock times)
    buf2 = io.StringIO()
    res2 = R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=buf2)
    plain = buf2.getvalue().splitlines()
    assert "2-RDM" not in buf2.getvalue() and "two_rdm" not in res2
    stage = set(range(lines.index(marks[0]) - 1, lines.index(marks[3]) + 1))      # the stage's lines and the blank one in front
    rest = [l for k, l in enumerate(lines) if k not in stage]
    assert rest[:-1] == plain[:-1] and rest[-1].startswith("sqmc_amd: variational stage") and plain[-1].startswith("sqmc_amd: variational stage")
    assert res2["states"] == res["states"]
