"""The transition-density-matrix entries of the HIP library (sqmc_gpu_hci_1tdm, sqmc_gpu_hci_2tdm), GpuChem.one_tdm / two_tdm, the host
layer around them and the --transition-rdm stage of the deck runner against tests/tdm_checker.py, which shares nothing with the
library.  Every comparison bound of an entry is the checker's derived rounding bound; exact zeros, symmetries, the swap identity, the
equality with the density-matrix doors and reproducibility are compared with == or on the bytes.  The Gram kernel gives an entry to a
wavefront (64 lanes) or a block (256 threads), the record sort works on tiles of 1024 and the one-body kernel on chunks of 1024
determinants: the list sizes straddle them."""
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
from tests import orbopt_checker as OC       # noqa: E402
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402
from tests import rdm2_checker as R2         # noqa: E402
from tests import tdm_checker as TC          # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
OK, BAD_ARG, ERR_HIP, UNSUPPORTED = 0, -1, -2, -3
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
SAMPLED = SIZES[-3:]
V = C.c_void_p


def _arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


def _vector(rng, n, offset):
    """random, normalised, and every seventh coefficient from `offset` an exact zero (lists of three and more)"""
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    if n >= 3:
        for k in range(offset % 7, n, 7):
            c[k] = 0.0
    s = math.sqrt(math.fsum(x * x for x in c))
    return [x / s for x in c]


def _pair(rng, n):
    """independent bra and ket, their exact zeros at different offsets"""
    return _vector(rng, n, 1), _vector(rng, n, 4)


def _dyadic(rng, n):
    """integers / 1024: sums and differences of two such vectors are exact"""
    return [rng.randrange(-1024, 1025) / 1024.0 for _ in range(n)]


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


_CHEM, _SD, _CASE = {}, {}, {}


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


def _check(g, dets, bra, ket, norb, tag="", sampled=False, seed=0, blocks="all"):
    """the device's blocks and one-body matrix of a list against the checker: every entry, or (sampled) a few thousand seeded two-body
    entries with terms plus the whole-array zero pattern from the entries the checker's pass reaches"""
    up, dn = _arrays(dets)
    got = g.two_tdm(up, dn, bra, ket, blocks)
    names = tuple(got)
    if sampled:
        exp = TC.two_tdm(dets, bra, ket, norb, {b: _Every8th(seed) for b in R2.BLOCKS})
        sample = {b: set(exp.terms[b]) for b in R2.BLOCKS}
        assert 3000 <= sum(len(sample[b]) for b in R2.BLOCKS) <= 30000, {b: len(sample[b]) for b in R2.BLOCKS}
    else:
        sample, exp = None, TC.two_tdm(dets, bra, ket, norb)
    fails, worst, seen = R2.compare(exp, got, names, sample)
    assert not fails, fails[:4]
    for b in names:                              # every entry no pair of determinants reaches is exactly +0.0
        rest = got[b][~_mask(exp.reached[b], norb)]
        assert np.count_nonzero(rest) == 0 and not np.any(np.signbit(rest)), b
    one, exp1 = g.one_tdm(up, dn, bra, ket), TC.one_tdm(dets, bra, ket, norb)
    fails1, worst1 = RC.compare(exp1, one)
    print("%s n = %d: %d two-body entries compared, worst |delta| / bound = %.3f; one-body worst %.3f" % (tag, len(dets), seen, worst, worst1))
    assert not fails1, fails1[:4]
    return got, exp, one, exp1


# ---------------------------------------------------------------------------------------------- 1. entries against the checker
@pytest.mark.parametrize("kind", ["sd", "neighbours"])
@pytest.mark.parametrize("n", SIZES)
def test_entries_chem(dev, n, kind):
    """C2, (nelec, nup) = (8, 4), 26 orbitals: HF + singles + doubles, and lists grown by single moves"""
    h, g, _ = _chem(dev)
    rng = random.Random(3000 + n + (0 if kind == "sd" else 50000))
    dets = _sd_list(h, rng, n) if kind == "sd" else _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, n)
    bra, ket = _pair(rng, n)
    got, exp, one, exp1 = _check(g, dets, bra, ket, h.norb, tag=kind, sampled=n in SAMPLED, seed=n)
    ovl, mass = TC.overlap(bra, ket), math.fsum(abs(a * b) for a, b in zip(bra, ket))
    for b, want in (("aa", 12), ("bb", 12), ("ab", 16)):
        tr = math.fsum(float(got[b][p, q, p, q]) for p in range(h.norb) for q in range(h.norb))
        assert abs(tr - want * ovl) <= PC.rounding_bound(n, want * mass) + 26 * 26 * RC.U * want * mass, (b, tr)
    tr = math.fsum(float(one[p, p]) for p in range(h.norb))
    assert abs(tr - 8 * ovl) <= math.fsum(exp1.bound(p, p) for p in range(h.norb)) + (26 + 2 * n) * RC.U * 8 * mass


# ---------------------------------------------------------------------------------------------- 2. electron-count edges
@pytest.mark.parametrize("nup,ndn", [(1, 3), (3, 0), (1, 1), (3, 1)])
def test_electron_count_edges(dev, nup, ndn):
    from sqmc_amd import host as H
    h = H.HubbardHost(4, 4, True, nup, ndn)
    g = h.gpu()
    try:
        rng = random.Random(10 * nup + ndn)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, 70)
        bra, ket = _pair(rng, len(dets))
        got, exp, one, _ = _check(g, dets, bra, ket, h.norb, tag="nup=%d ndn=%d" % (nup, ndn))
        for b, live in (("aa", nup >= 2), ("bb", ndn >= 2), ("ab", nup >= 1 and ndn >= 1)):
            assert (np.count_nonzero(got[b]) > 0) == live, b
            assert live or (not np.any(np.signbit(got[b])) and got[b].shape == (16,) * 4)
        assert np.count_nonzero(one) > 20 and not np.array_equal(one, one.T)
    finally:
        g.close()


def test_single_determinant(dev):
    h, g, _ = _chem(dev)
    b_, k_ = 0.75, -0.5
    got = g.two_tdm([h.hf_up], [h.hf_dn], [b_], [k_])
    ou, od = RC.occupation(int(h.hf_up)), RC.occupation(int(h.hf_dn))
    for b, left, right in (("aa", ou, ou), ("bb", od, od), ("ab", ou, od)):
        want = np.zeros((h.norb,) * 4)
        for p in left:
            for q in right:
                if b == "ab" or p != q:
                    want[p, q, p, q] = b_ * k_
                    if b != "ab":
                        want[p, q, q, p] = -(b_ * k_)
        assert np.array_equal(got[b], want) and not np.any(np.signbit(got[b][want == 0.0])), b
    one = g.one_tdm([h.hf_up], [h.hf_dn], [b_], [k_])
    want = np.zeros((h.norb, h.norb))
    for p in range(h.norb):
        want[p, p] = (p in ou) * (b_ * k_) + (p in od) * (b_ * k_)
    assert np.array_equal(one, want)


# ---------------------------------------------------------------------------------------------- 3. bits 0 and 63, the two-pass order
def _lattice_blocks(g, dets, bra, ket, min_live, exact=None):
    """one block per call (134 MB each) and the one-body matrix of a 64-site list against the checker"""
    up, dn = _arrays(dets)
    exp = TC.two_tdm(dets, bra, ket, 64)
    for b in R2.BLOCKS:
        got = g.two_tdm(up, dn, bra, ket, b)
        assert list(got) == [b]
        a = got[b]
        worst = 0.0
        for idx in exp.terms[b]:
            x, want, bd = float(a[idx]), exp.value(b, idx), exp.bound(b, idx)
            assert abs(x - want) <= bd, (b, idx, x, want)
            worst = max(worst, abs(x - want) / bd if bd else 0.0)
        live = sum(1 for idx in exp.terms[b] if exp.value(b, idx) != 0.0)
        print("8x8 %s: %d entries with terms, worst |delta| / bound = %.3f" % (b, len(exp.terms[b]), worst))
        assert np.count_nonzero(a) == live and live > min_live, (b, live)
        assert not np.any(np.signbit(a[a == 0.0]))
        if exact is not None:
            exact(b, a, exp)
        del got, a
    one = g.one_tdm(up, dn, bra, ket)
    fails, _ = RC.compare(TC.one_tdm(dets, bra, ket, 64), one)
    assert not fails, fails[:4]
    return one


def test_bits_0_and_63_on_the_8x8_lattice(dev):
    from sqmc_amd import host as H
    h = H.HubbardHost(8, 8, True, 3, 2)
    g = h.gpu()
    try:
        a_up, dn0 = (1 << 0) | (1 << 5) | (1 << 9), (1 << 62) | (1 << 3)
        dets = [(a_up, dn0), ((a_up ^ 1) | (1 << 63), dn0), (a_up, (1 << 63) | (1 << 3)), (a_up, (1 << 63) | (1 << 0)),
                ((1 << 62) | (1 << 5) | (1 << 9), dn0), ((1 << 63) | (1 << 62) | (1 << 61), dn0), ((1 << 63) | (1 << 5) | (1 << 0), (1 << 63) | (1 << 0))]
        bra, ket = [0.5, -0.4, 0.3, 0.45, -0.35, 0.4, 0.25], [0.125, 0.5, -0.25, 0.75, 0.375, -0.5, 0.625]

        def exact(b, a, exp):
            if b == "ab":
                assert exp.count("ab", (63, 63, 63, 63)) == 1 and a[63, 63, 63, 63] == 0.25 * 0.625 and a[0, 0, 0, 0] == 0.45 * 0.75 + 0.25 * 0.625
        one = _lattice_blocks(g, dets, bra, ket, 20, exact)
        assert one[0, 63] != 0.0 and one[63, 0] != 0.0 and one[0, 63] != one[63, 0]      # determinants 0 and 1: the up electron moves 0 <-> 63
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
        bra, ket = _pair(rng, len(dets))
        up, dn = _arrays(dets)

        def exact(b, a, exp):
            again = g.two_tdm(up[::-1], dn[::-1], bra[::-1], ket[::-1], b)[b]
            assert a.tobytes(order="F") == again.tobytes(order="F")
        _lattice_blocks(g, dets, bra, ket, 200, exact)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 4. heavy columns
def test_heavy_columns_take_the_block_owner(dev):
    """1050 determinants, two up strings {0,1,2,3} and {0,1,2,4} times 525 random dn strings: the aa columns of the pairs inside them
    hold 1050 or 525 records, past the 512 at which an entry goes to a 256-thread block, and the ab and bb columns stay short, so one
    call runs k_tdm2_gram<256> and <64>.  T_aa[2,3,2,4] and T_aa[2,4,2,3] are the two accumulators of one block owner: 525 terms
    each, and different numbers"""
    h, g, _ = _chem(dev)
    rng = random.Random(8)
    dns = set()
    while len(dns) < 525:
        dns.add(sum(1 << k for k in rng.sample(range(h.norb), 4)))
    dets = [(u, d) for u in (0b01111, 0b10111) for d in sorted(dns)]
    rng.shuffle(dets)
    bra, ket = _pair(rng, len(dets))
    up, dn = _arrays(dets)
    got = g.two_tdm(up, dn, bra, ket)
    five = [(p, q, r, s) for p in range(5) for q in range(5) for r in range(5) for s in range(5)]
    sample = {"aa": set(five), "bb": set(five) | {tuple(rng.randrange(26) for _ in range(4)) for _ in range(300)},
              "ab": {(p, rng.randrange(26), r, rng.randrange(26)) for p in range(5) for r in range(5) for _ in range(40)}}
    exp = TC.two_tdm(dets, bra, ket, h.norb, sample)
    fails, worst, seen = R2.compare(exp, got, R2.BLOCKS, sample)
    print("heavy: %d entries compared, worst |delta| / bound = %.3f" % (seen, worst))
    assert not fails, fails[:4]
    assert exp.count("aa", (2, 3, 2, 4)) == 525 and exp.count("aa", (2, 4, 2, 3)) == 525 and exp.count("aa", (0, 1, 0, 1)) == 1050
    assert got["aa"][2, 3, 2, 4] != 0.0 and got["aa"][2, 4, 2, 3] != 0.0 and got["aa"][2, 3, 2, 4] != got["aa"][2, 4, 2, 3]
    assert sum(exp.count("ab", k) > 0 for k in sample["ab"]) > 50
    for b in R2.BLOCKS:
        assert np.count_nonzero(got[b][~_mask(exp.reached[b], h.norb)]) == 0
    again, swapped = g.two_tdm(up, dn, bra, ket), g.two_tdm(up, dn, ket, bra)
    for b in R2.BLOCKS:
        assert again[b].tobytes(order="F") == got[b].tobytes(order="F")
        assert np.array_equal(swapped[b].transpose(2, 3, 0, 1), got[b])
    fails1, _ = RC.compare(TC.one_tdm(dets, bra, ket, h.norb), g.one_tdm(up, dn, bra, ket))       # two chunks of determinants
    assert not fails1, fails1[:4]


# ---------------------------------------------------------------------------------------------- 5. exact properties
def _case(dev, n=300):
    """one list of the C2 fixture with two vectors, its device blocks and one-body matrix, shared by the tests below"""
    if n not in _CASE:
        h, g, HH = _chem(dev)
        rng = random.Random(5252 + n)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, n // 2) if n > 100 else []
        dets = dets + [d for d in _sd_list(h, rng, n) if d not in set(dets)][:n - len(dets)]
        bra, ket = _pair(rng, len(dets))
        up, dn = _arrays(dets)
        _CASE[n] = dict(dets=dets, bra=np.array(bra), ket=np.array(ket), up=up, dn=dn, got=g.two_tdm(up, dn, bra, ket), one=g.one_tdm(up, dn, bra, ket))
    return _CASE[n]


def _same(a, b):
    return a.tobytes(order="F") == b.tobytes(order="F")


def test_same_bits_again_shuffled_alone_and_on_a_second_context(dev):
    h, g, _ = _chem(dev)
    cs = _case(dev)
    up, dn, bra, ket, got, one = cs["up"], cs["dn"], cs["bra"], cs["ket"], cs["got"], cs["one"]
    order = np.random.RandomState(5).permutation(len(bra))
    g2 = h.gpu()
    try:
        runs = [(g.two_tdm(up, dn, bra, ket), g.one_tdm(up, dn, bra, ket)),
                (g.two_tdm(up[order], dn[order], bra[order], ket[order]), g.one_tdm(up[order], dn[order], bra[order], ket[order])),
                (g2.two_tdm(up, dn, bra, ket), g2.one_tdm(up, dn, bra, ket))]
    finally:
        g2.close()
    for two, o in runs:
        assert _same(o, one) and all(_same(two[b], got[b]) for b in R2.BLOCKS)
    for b in R2.BLOCKS:
        alone = g.two_tdm(up, dn, bra, ket, b)
        assert list(alone) == [b] and _same(alone[b], got[b]), b
    two = g.two_tdm(up, dn, bra, ket, ("aa", "ab"))
    assert sorted(two) == ["aa", "ab"] and all(_same(two[b], got[b]) for b in two)


def test_swap_transposes_and_equal_vectors_give_the_density_matrices(dev):
    h, g, _ = _chem(dev)
    cs = _case(dev)
    up, dn, bra, ket, got, one = cs["up"], cs["dn"], cs["bra"], cs["ket"], cs["got"], cs["one"]
    swapped, one_s = g.two_tdm(up, dn, ket, bra), g.one_tdm(up, dn, ket, bra)
    for b in R2.BLOCKS:
        assert np.count_nonzero(got[b]) > 1000 and not np.array_equal(got[b], got[b].transpose(2, 3, 0, 1))
        assert _same(got[b], np.asfortranarray(swapped[b].transpose(2, 3, 0, 1))), b
    assert _same(one, np.asfortranarray(one_s.T)) and not np.array_equal(one, one.T)
    for c in (bra, ket):
        tt, rr = g.two_tdm(up, dn, c, c), g.two_rdm(up, dn, c)
        assert all(_same(tt[b], rr[b]) for b in R2.BLOCKS)
        t1, r1 = g.one_tdm(up, dn, c, c), g.one_rdm(up, dn, c)
        upper = np.triu(r1)
        assert _same(t1, np.asfortranarray(upper + np.triu(r1, 1).T))          # [p, r] and [r, p]: the bits of one_rdm[min, max]
        assert np.count_nonzero(np.triu(r1, 1)) > 50


def test_antisymmetry_scaling_and_zeros(dev):
    h, g, _ = _chem(dev)
    cs = _case(dev)
    up, dn, bra, ket, got, one = cs["up"], cs["dn"], cs["bra"], cs["ket"], cs["got"], cs["one"]
    norb, n = h.norb, len(bra)
    for b in ("aa", "bb"):
        assert np.array_equal(got[b], -got[b].transpose(1, 0, 2, 3)) and np.array_equal(got[b], -got[b].transpose(0, 1, 3, 2)), b
        assert np.array_equal(got[b], got[b].transpose(1, 0, 3, 2))
        for p in range(norb):
            assert np.count_nonzero(got[b][p, p]) == 0 and np.count_nonzero(got[b][:, :, p, p]) == 0
    doubled, one_d = g.two_tdm(up, dn, 2.0 * bra, ket), g.one_tdm(up, dn, 2.0 * bra, ket)
    assert all(_same(doubled[b], 2.0 * got[b]) for b in R2.BLOCKS) and _same(one_d, 2.0 * one)
    for two, o in ((g.two_tdm(up, dn, bra, np.zeros(n)), g.one_tdm(up, dn, bra, np.zeros(n))),
                   (g.two_tdm(up, dn, np.zeros(n), ket), g.one_tdm(up, dn, np.zeros(n), ket))):
        for a in list(two.values()) + [o]:
            assert np.count_nonzero(a) == 0 and not np.any(np.signbit(a))
    neg, one_n = g.two_tdm(up, dn, bra, -ket), g.one_tdm(up, dn, bra, -ket)
    for a in list(got.values()) + list(neg.values()) + [one, one_n]:
        assert not np.any(np.signbit(a[a == 0.0]))                    # no -0.0 anywhere
    assert all(np.array_equal(neg[b], -got[b]) for b in R2.BLOCKS) and np.array_equal(one_n, -one)
    # bra on one half of the list, ket on the other: no determinant carries both, so every diagonal entry is an exact +0.0
    half = np.arange(n) < n // 2
    b1, k1 = np.where(half, bra, 0.0), np.where(half, 0.0, ket)
    two, o = g.two_tdm(up, dn, b1, k1), g.one_tdm(up, dn, b1, k1)
    for b in R2.BLOCKS:
        d = np.einsum("pqpq->pq", two[b])
        assert np.count_nonzero(d) == 0 and not np.any(np.signbit(d)) and np.count_nonzero(two[b]) > 100, b
    assert np.count_nonzero(np.diag(o)) == 0 and not np.any(np.signbit(np.diag(o))) and np.count_nonzero(o) > 10


def test_orbital_symmetries_filter(dev):
    h, g, _ = _chem(dev)
    cs = _case(dev)
    sym = np.asarray(h.orbsym[1:h.norb + 1], np.int32)
    one = cs["one"]
    fil = g.one_tdm(cs["up"], cs["dn"], cs["bra"], cs["ket"], sym)
    same = sym[:, None] == sym[None, :]
    assert np.count_nonzero(fil[~same]) == 0 and not np.any(np.signbit(fil[~same]))
    assert fil[same].tobytes() == one[same].tobytes() and np.count_nonzero(one[~same]) > 10
    exp = TC.one_tdm(cs["dets"], cs["bra"].tolist(), cs["ket"].tolist(), h.norb, sym.tolist())
    assert not RC.compare(exp, fil)[0]


# ---------------------------------------------------------------------------------------------- 6. identities on the device's output
def _device_energy(HH, one, d, ovl):
    """(<bra|H|ket>, sum |term|) from the device's matrices with the checker's integrals, summed with fsum"""
    vals = [HH.const * ovl]
    for p, r in np.argwhere(one != 0.0).tolist():
        vals.append(HH.t(p, r) * float(one[p, r]))
    for b in R2.BLOCKS:
        w = 1.0 if b == "ab" else 0.5
        for p, q, r, s in np.argwhere(d[b] != 0.0).tolist():
            vals.append(w * HH.v(p, r, q, s) * float(d[b][p, q, r, s]))
    return math.fsum(vals), math.fsum(abs(x) for x in vals)


def _plan_element(sqmc_amd, H, g, up, dn, bra, ket):
    """bra . (H ket) from the library's resident plan of the list"""
    order = H.sort_dets(up, dn)
    plan, _, _ = sqmc_amd.SpmvPlan.from_dets(g, up[order], dn[order])
    try:
        return float(np.dot(np.asarray(bra)[order], plan.apply(np.asarray(ket)[order])))
    finally:
        plan.close()


def test_identities_chem(dev):
    from sqmc_amd import host as H
    import sqmc_amd
    h, g, HH = _chem(dev)
    cs = _case(dev, 120)
    dets, got, one = cs["dets"], cs["got"], cs["one"]
    bra, ket = cs["bra"].tolist(), cs["ket"].tolist()
    norb, n, ovl = h.norb, len(dets), TC.overlap(bra, ket)
    exp2, exp1 = TC.two_tdm(dets, bra, ket, norb), TC.one_tdm(dets, bra, ket, norb)
    assert not R2.compare(exp2, got)[0] and not RC.compare(exp1, one)[0]
    sf = H.spin_free_two_rdm(got)
    # partial trace = (N - 1) times the device's own one-body matrix (one[p, r] = <bra| a+_r a_p |ket>)
    worst = 0.0
    for p in range(norb):
        for r in range(norb):
            want, bw = R2.partial_trace(exp2, p, r, 8)
            x = math.fsum(float(sf[p, q, r, q]) for q in range(norb))
            bound = 2 * bw + 7 * exp1.bound(r, p) + 8 * RC.U * abs(want)
            assert abs(x - 7 * float(one[r, p])) <= bound, (p, r, x, 7 * one[r, p], bound)
            worst = max(worst, abs(x - 7 * float(one[r, p])) / bound if bound else 0.0)
    assert not np.array_equal(np.einsum("pqrq->pr", sf), np.einsum("pqrq->rp", sf))
    # <bra|H|ket>: the device's matrices with the checker's integrals against the checker's sum over all pairs
    e_chk, b_chk = TC.energy(HH, exp1, exp2, ovl)
    want, bw, sa = TC.expectation(HH, dets, bra, ket)
    e_dev, sa_dev = _device_energy(HH, one, got, ovl)
    print("identities: partial trace worst %.3f of its bound; <bra|H|ket> (device matrices) = %.12f, all pairs = %.12f, |delta| = %.3g, bound = %.3g"
          % (worst, e_dev, want, abs(e_dev - want), 2 * b_chk + bw))
    assert abs(e_dev - want) <= 2 * b_chk + bw
    assert abs(e_chk - want) <= b_chk + bw
    # host.rdm_energy: the library's own integrals and numpy's sums over all norb^4 entries; the overlap from the trace
    assert abs(H.transition_overlap(h, one) - ovl) <= math.fsum(exp1.bound(p, p) for p in range(norb)) / 8 + (norb + 2 * n) * RC.U * math.fsum(abs(a * b) for a, b in zip(bra, ket))
    e_host = H.rdm_energy(h, one, sf)
    assert abs(e_host - want) <= 2 * b_chk + bw + (norb ** 4) * RC.U * sa_dev
    # bra . (H ket) from the library's resident plan of the same list: pins the sign convention to h_any
    e_plan = _plan_element(sqmc_amd, H, g, cs["up"], cs["dn"], bra, ket)
    print("bra.H ket = %.12f, |device matrices - plan| = %.3g" % (e_plan, abs(e_dev - e_plan)))
    assert abs(e_plan - want) <= bw + 4 * n * RC.U * sa
    assert abs(e_dev - e_plan) <= 2 * b_chk + 2 * bw + 4 * n * RC.U * sa
    assert abs(want) > 1e-3
    # <bra|S^2|ket> against the polarised checker value
    ex = [float(got["ab"][q, p, p, q]) for p in range(norb) for q in range(norb)]
    s_dev = math.fsum([(0.0 + 0.0 + 4) * ovl] + [-x for x in ex])
    s_chk, bp = TC.s_squared_polarised(dets, bra, ket, norb), TC.s_squared_polarised_bound(dets, bra, ket, norb)
    bs = math.fsum(exp2.bound("ab", (q, p, p, q)) for p in range(norb) for q in range(norb)) + (norb * norb + n) * RC.U * (4 * abs(ovl) + math.fsum(abs(x) for x in ex))
    assert abs(s_dev - s_chk) <= bs + bp, (s_dev, s_chk, bs + bp)
    assert abs(H.s_squared(h, got["ab"], ovl) - s_chk) <= 2 * bs + bp
    assert abs(s_chk) > 1e-4


def test_identities_hubbard(dev):
    """4 x 4 periodic lattice: U sum_i T_ab[i,i,i,i] - t sum over bonds of the one-body matrix against the plan's bra . H ket"""
    from sqmc_amd import host as H
    import sqmc_amd
    t, U = 1.0, 4.0
    h = H.HubbardHost(4, 4, True, 3, 3, t, U)
    HH = PC.HubbardH(4, 4, True, t, U)
    g = h.gpu()
    try:
        rng = random.Random(16)
        dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), 16, 150)
        bra, ket = _pair(rng, len(dets))
        up, dn = _arrays(dets)
        got, exp2, one, exp1 = _check(g, dets, bra, ket, 16, tag="hubbard 4x4")
        # partial trace = (N - 1) times the device's own one-body matrix, N = 6: ties the (p, r) / (r, p) orientation of the one-body
        # kernel to the two-body blocks on a context that is not chem
        sf = H.spin_free_two_rdm(got)
        for p in range(16):
            for r in range(16):
                want_pt, bw_pt = R2.partial_trace(exp2, p, r, 6)
                x = math.fsum(float(sf[p, q, r, q]) for q in range(16))
                bound_pt = 2 * bw_pt + 5 * exp1.bound(r, p) + 6 * RC.U * abs(want_pt)
                assert abs(x - 5 * float(one[r, p])) <= bound_pt, (p, r, x, 5 * one[r, p], bound_pt)
        assert not np.array_equal(np.einsum("pqrq->pr", sf), np.einsum("pqrq->rp", sf))
        inter = [U * float(got["ab"][i, i, i, i]) for i in range(16)]
        hop = [-t * (float(one[i, j]) + float(one[j, i])) for i, j in HH.bonds]
        e_dev = math.fsum(inter + hop)
        bound = U * math.fsum(exp2.bound("ab", (i, i, i, i)) for i in range(16)) + t * math.fsum(exp1.bound(i, j) + exp1.bound(j, i) for i, j in HH.bonds)
        bound += 64 * RC.U * math.fsum(abs(x) for x in inter + hop)
        want, bw, sa = TC.expectation(HH, dets, bra, ket)
        assert abs(e_dev - want) <= bound + bw, (e_dev, want, bound + bw)
        e_plan = _plan_element(sqmc_amd, H, g, up, dn, bra, ket)
        print("hubbard: U sum T_ab - t sum T1 = %.12f, bra.H ket = %.12f, all pairs = %.12f" % (e_dev, e_plan, want))
        assert abs(e_dev - e_plan) <= bound + 2 * bw + 4 * len(bra) * RC.U * sa
        assert abs(H.rdm_energy(h, one, H.spin_free_two_rdm(got)) - want) <= bound + bw + 16 ** 4 * RC.U * sa
        assert abs(math.fsum(inter)) > 1e-4 and abs(want) > 1e-4
        ex = [float(got["ab"][q, p, p, q]) for p in range(16) for q in range(16)]
        ovl = TC.overlap(bra, ket)
        s_dev = math.fsum([3 * ovl] + [-x for x in ex])
        bs = math.fsum(exp2.bound("ab", (q, p, p, q)) for p in range(16) for q in range(16)) + (256 + len(bra)) * RC.U * (3 * abs(ovl) + math.fsum(abs(x) for x in ex))
        assert abs(s_dev - TC.s_squared_polarised(dets, bra, ket, 16)) <= bs + TC.s_squared_polarised_bound(dets, bra, ket, 16)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 7. the orbital-CI coupling
def _dense_bounds(exp, norb):
    """(values, bounds) of an Rdm2 as dense arrays per block"""
    out = {}
    for b in R2.BLOCKS:
        v, bd = np.zeros((norb,) * 4), np.zeros((norb,) * 4)
        for idx in exp.terms[b]:
            v[idx], bd[idx] = exp.value(b, idx), exp.bound(b, idx)
        out[b] = (v, bd)
    return out


def test_coupling_is_the_polarised_density_matrix_and_the_gradient_on_it(dev):
    from sqmc_amd import host as H
    h, g, _ = _chem(dev)
    rng = random.Random(77)
    n, norb = 120, h.norb
    dets = _neighbours(rng, (int(h.hf_up), int(h.hf_dn)), norb, n // 2)
    dets = dets + [d for d in _sd_list(h, rng, n) if d not in set(dets)][:n - len(dets)]
    c, v = _dyadic(rng, n), _dyadic(rng, n)
    plus, minus = [a + b for a, b in zip(c, v)], [a - b for a, b in zip(c, v)]
    assert all(float(np.float64(a) - np.float64(b)) == x for a, b, x in zip(plus, v, c))        # c +- v are exact
    up, dn = _arrays(dets)
    t2, t1 = g.two_tdm(up, dn, c, v), g.one_tdm(up, dn, c, v)
    gp, gm = g.two_rdm(up, dn, plus), g.two_rdm(up, dn, minus)
    dp, dm = g.one_rdm(up, dn, plus), g.one_rdm(up, dn, minus)
    e_cv, e_vc = _dense_bounds(TC.two_tdm(dets, c, v, norb), norb), _dense_bounds(TC.two_tdm(dets, v, c, norb), norb)
    e_p, e_m = _dense_bounds(R2.two_rdm(dets, plus, norb), norb), _dense_bounds(R2.two_rdm(dets, minus, norb), norb)
    for b in R2.BLOCKS:
        sym = t2[b] + t2[b].transpose(2, 3, 0, 1)                     # T(c, v) + T(v, c): the swap identity is exact
        pol = (gp[b] - gm[b]) / 2                                     # the sum and the difference round once each: 2 U on either side
        bound = e_cv[b][1] + e_vc[b][1] + (e_p[b][1] + e_m[b][1]) / 2 + 2 * RC.U * (np.abs(sym) + np.abs(pol))
        bad = np.argwhere(~(np.abs(sym - pol) <= bound))
        assert len(bad) == 0, (b, bad[:4].tolist())
        assert np.count_nonzero(sym) > 1000 and np.count_nonzero(bound) > 1000
    o_cv, o_p, o_m = TC.one_tdm(dets, c, v, norb), RC.one_rdm(dets, plus, norb), RC.one_rdm(dets, minus, norb)
    for p in range(norb):
        for r in range(norb):
            bound = o_cv.bound(p, r) + o_cv.bound(r, p) + (o_p.bound(p, r) + o_m.bound(p, r)) / 2
            x, y = float(t1[p, r]) + float(t1[r, p]), (float(dp[p, r]) - float(dm[p, r])) / 2
            assert abs(x - y) <= bound + 2 * RC.U * (abs(x) + abs(y)), (p, r, x, y)
    # the coupling: the orbital gradient on the symmetrised transition matrices, against the numpy yardstick on the same matrices
    k = H.ci_orbital_coupling(g, up, dn, c, v)
    sf = H.spin_free_two_rdm(t2)
    D, G = t1 + t1.T, sf + sf.transpose(2, 3, 0, 1)
    ref = H.orbital_gradient_host(h, D, G)["gradient"]
    hh, ee, _ = H.dense_integrals(h)
    fabs = OC.fock_abs(hh, ee, D, G)
    worst = 0.0
    for p in range(norb):
        for q in range(norb):
            if p != q:
                bd = 2 * OC.gradient_bound(norb, fabs, p, q)
                assert abs(k[p, q] - ref[p, q]) <= bd, (p, q, k[p, q], ref[p, q], bd)
                worst = max(worst, abs(k[p, q] - ref[p, q]) / bd)
    print("coupling: max |k| = %.6g, worst |door - yardstick| / bound = %.3f" % (float(np.max(np.abs(k))), worst))
    assert np.array_equal(k, -k.T) and np.count_nonzero(k) > 20 and float(np.max(np.abs(k))) > 1e-3


# ---------------------------------------------------------------------------------------------- 8. refusals and scratch
def _raw2(L, ctx, u, d, bra, ket, blocks, outs):
    u, d = np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(d, np.uint64)
    bra, ket = np.ascontiguousarray(bra, np.float64), np.ascontiguousarray(ket, np.float64)
    L.sqmc_gpu_hci_2tdm.argtypes = [V, C.c_int64, V, V, V, V, C.c_int32, V, V, V]
    return L.sqmc_gpu_hci_2tdm(ctx.h, len(u), u.ctypes.data_as(V), d.ctypes.data_as(V), bra.ctypes.data_as(V), ket.ctypes.data_as(V), blocks,
                               *[None if a is None else a.ctypes.data_as(V) for a in outs])


def _raw1(L, ctx, u, d, bra, ket, sym, out):
    u, d = np.ascontiguousarray(u, np.uint64), np.ascontiguousarray(d, np.uint64)
    bra, ket = np.ascontiguousarray(bra, np.float64), np.ascontiguousarray(ket, np.float64)
    sym = None if sym is None else np.ascontiguousarray(sym, np.int32)
    L.sqmc_gpu_hci_1tdm.argtypes = [V, C.c_int64, V, V, V, V, V, V]
    return L.sqmc_gpu_hci_1tdm(ctx.h, len(u), u.ctypes.data_as(V), d.ctypes.data_as(V), bra.ctypes.data_as(V), ket.ctypes.data_as(V),
                               None if sym is None else sym.ctypes.data_as(V), out.ctypes.data_as(V))


def test_refusals_leave_the_outputs_untouched(dev):
    from sqmc_amd import host as H
    h, g, _ = _chem(dev)
    L = g.L
    rng = random.Random(77)
    dets = _sd_list(h, rng, 100)
    bra, ket = _pair(rng, 100)
    up, dn = _arrays(dets)
    outs, out1 = [np.full(h.norb ** 4, 7.25) for _ in range(3)], np.full(h.norb ** 2, 7.25)
    untouched = lambda: all(bool(np.all(a == 7.25)) for a in outs + [out1])

    def both(u, d, b, k, code):
        assert _raw2(L, g, u, d, b, k, 7, outs) == code and untouched()
        assert _raw1(L, g, u, d, b, k, None, out1) == code and untouched()
    both(np.concatenate((up, up[41:42])), np.concatenate((dn, dn[41:42])), np.concatenate((bra, [0.1])), np.concatenate((ket, [0.2])), BAD_ARG)
    wrong = up.copy(); wrong[5] |= np.uint64(1 << 20) if not int(wrong[5]) >> 20 & 1 else np.uint64(1 << 21)
    both(wrong, dn, bra, ket, BAD_ARG)
    beyond = up.copy(); beyond[3] = (int(beyond[3]) & ~(1 << PC._bits(int(beyond[3]))[0])) | (1 << 40)
    both(beyond, dn, bra, ket, BAD_ARG)
    both(up[:0], dn[:0], bra[:0], ket[:0], BAD_ARG)
    for blocks in (0, 8, -1):
        assert _raw2(L, g, up, dn, bra, ket, blocks, outs) == BAD_ARG and untouched()
    for k in range(3):
        holes = [None if j == k else outs[j] for j in range(3)]
        assert _raw2(L, g, up, dn, bra, ket, 7, holes) == BAD_ARG and untouched()
        assert _raw2(L, g, up, dn, bra, ket, 1 << k, holes) == BAD_ARG and untouched()
    assert _raw1(L, g, up, dn, bra, ket, [0] * 25 + [256], out1) == BAD_ARG and untouched()
    ts = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1)
    gt = ts.gpu()
    try:
        assert _raw2(L, gt, up, dn, bra, ket, 7, outs) == UNSUPPORTED and untouched()
        assert _raw1(L, gt, up, dn, bra, ket, None, out1) == UNSUPPORTED and untouched()
        for call in (lambda: gt.two_tdm(up, dn, bra, ket), lambda: gt.one_tdm(up, dn, bra, ket)):
            with pytest.raises(dev.SqmcGpuError) as e:
                call()
            assert e.value.code == UNSUPPORTED
    finally:
        gt.close()
    hk = H.HubbardKHost(4, 4, 2, 2, 1.0, 4.0, space_sym=True, z=1, p=1, start=(17, 3))
    gk = hk.gpu()
    try:
        small, small1 = [np.full(16 ** 4, 7.25) for _ in range(3)], np.full(256, 7.25)
        assert _raw2(L, gk, [hk.hf_up], [hk.hf_dn], [1.0], [1.0], 7, small) == UNSUPPORTED and all(bool(np.all(a == 7.25)) for a in small)
        assert _raw1(L, gk, [hk.hf_up], [hk.hf_dn], [1.0], [1.0], None, small1) == UNSUPPORTED and bool(np.all(small1 == 7.25))
    finally:
        gk.close()
    with pytest.raises(ValueError):
        g.two_tdm(up, dn, bra, ket, "ba")
    with pytest.raises(ValueError):
        g.two_tdm(up, dn, bra, ket[:-1])
    # a good call afterwards, with a block left out and its pointer null
    assert _raw2(L, g, up, dn, bra, ket, 5, [outs[0], None, outs[2]]) == OK and bool(np.all(outs[1] == 7.25))
    ref = g.two_tdm(up, dn, bra, ket)
    assert outs[0].tobytes() == ref["aa"].tobytes(order="F") and outs[2].tobytes() == ref["ab"].tobytes(order="F")
    assert _raw1(L, g, up, dn, bra, ket, None, out1) == OK and out1.tobytes() == g.one_tdm(up, dn, bra, ket).tobytes(order="F")


def test_key_bits_and_record_count_refusals(dev):
    """57 up and 57 dn electrons on the 8 x 8 lattice: the determinant space, C(64,57)^2 = 3.9e17, fits 63 bits, while the
    intermediates of the ab block live in C(64,56)^2 = 1.96e19 > 2^64 = 1.84e19, so that block is refused for its key bits; the aa
    block's C(64,55) C(64,57) = 1.72e19 fits, and with R = C(57,2) = 1596 records per determinant a list of ceil((2^32 - 1) / 1596)
    determinants reaches the record limit.  Both checks stand in front of the list's upload: nothing is taken from the device"""
    from sqmc_amd import host as H
    assert math.comb(64, 57) ** 2 < 2 ** 63 and math.comb(64, 56) ** 2 > 2 ** 64 and math.comb(64, 55) * math.comb(64, 57) <= 2 ** 64
    h = H.HubbardHost(8, 8, True, 57, 57)
    g = h.gpu()
    try:
        L = g.L
        L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]

        def counters():
            a = [C.c_int64() for _ in range(4)]
            assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 0) == OK
            return tuple(x.value for x in a)
        out = np.full(64 ** 4, 7.25)
        base = counters()
        u, d = [h.hf_up], [h.hf_dn]
        for blocks, outs in ((4, [None, None, out]), (6, [None, out, out]), (5, [out, None, out])):
            assert _raw2(L, g, u, d, [1.0], [0.5], blocks, outs) == UNSUPPORTED, blocks
            assert b"64 bits" in L.sqmc_gpu_last_error() and bool(np.all(out == 7.25)) and counters() == base
        with pytest.raises(dev.SqmcGpuError) as e:
            g.two_tdm(u, d, [1.0], [0.5], "ab")
        assert e.value.code == UNSUPPORTED
        # the record limit on the aa block, which fits its key bits: n_var R >= 2^32 - 1
        R = math.comb(57, 2)
        n = -(-(2 ** 32 - 1) // R)
        assert (n - 1) * R < 2 ** 32 - 1 <= n * R and n * R < 2 ** 33
        uu, dd, cc = np.full(n, h.hf_up, np.uint64), np.full(n, h.hf_dn, np.uint64), np.full(n, 0.5)
        assert _raw2(L, g, uu, dd, cc, cc, 1, [out, None, None]) == UNSUPPORTED
        assert b"records" in L.sqmc_gpu_last_error() and bool(np.all(out == 7.25)) and counters() == base
        # one determinant fewer passes that check: the list is then refused for its repeated determinant, after its upload
        assert _raw2(L, g, uu[:-1], dd[:-1], cc[:-1], cc[:-1], 1, [out, None, None]) == BAD_ARG
        assert b"twice" in L.sqmc_gpu_last_error() and bool(np.all(out == 7.25)) and counters()[:2] == base[:2]
        # and the block that fits is computed
        ok = g.two_tdm(u, d, [1.0], [0.5], "aa")["aa"]
        assert np.count_nonzero(ok) == 2 * 57 * 56 and float(ok[0, 1, 0, 1]) == 0.5 and not np.any(np.signbit(ok[ok == 0.0]))
    finally:
        g.close()


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
    bra, ket = _pair(rng, 40)
    up, dn = _arrays(dets)
    sym = [int(x) for x in h.orbsym[1:h.norb + 1]]
    outs2, out1 = [np.full(h.norb ** 4, 7.25) for _ in range(3)], [np.full(h.norb ** 2, 7.25)]
    for name, outs, call, lo in (("2-TDM", outs2, lambda: _raw2(L, g, up, dn, bra, ket, 7, outs2), 20),
                                 ("1-TDM", out1, lambda: _raw1(L, g, up, dn, bra, ket, sym, out1[0]), 8)):
        base = counters()
        assert call() == OK
        first = [a.copy() for a in outs]
        after = counters()
        assert after[:2] == base[:2]
        takes = after[3] - base[3]
        assert lo <= takes <= 200, (name, takes)
        for a in outs:
            a[:] = 7.25
        for k in range(1, takes + 1):
            assert L.sqmc_gpu_debug_scratch_fail_at(k) == OK
            rc = call()
            L.sqmc_gpu_debug_scratch_fail_at(0)
            assert rc == ERR_HIP, (name, k, takes, rc, L.sqmc_gpu_last_error())
            assert counters()[:2] == base[:2], (name, k, "live allocations after a failed take")
            assert all(bool(np.all(a == 7.25)) for a in outs), (name, k, "a failed call wrote an output")
        assert call() == OK
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, first)) and counters()[:2] == base[:2]
        print("%s: %d takes, every early return balanced" % (name, takes))


# ---------------------------------------------------------------------------------------------- 9. host layer and deck
def test_host_layer_on_a_time_symmetrised_wavefunction(dev):
    """i_1sigma_g conventions, two states, one iteration at eps_var 5e-3: hci_transition_rdms against the doors on the hand-expanded
    list byte for byte, the union of two truncations against the checker, natural transition orbitals"""
    from sqmc_amd import host as H
    import copy
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    g = h.gpu()
    try:
        g.set_hb_tables(*h.hb_tables(g))
        up, dn, w, e, hist = H.hci_variational(h, g, 5e-3, n_states=2, max_iters=1)
    finally:
        g.close()
    assert 50 <= len(up) <= 1500, hist
    one, two = H.hci_transition_rdms(h, up, dn, w, 0, 1)
    du, dd, c0 = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
    du1, dd1, c1 = H.time_symmetrized_to_dets(up, dn, w[:, 1], h.z)
    assert np.array_equal(du, du1) and np.array_equal(dd, dd1) and len(du) > len(up)
    plain = copy.copy(h)
    plain.time_sym = False
    gp = plain.gpu()
    try:
        by_hand, one_hand = gp.two_tdm(du, dd, c0, c1), gp.one_tdm(du, dd, c0, c1)
        assert _same(one, one_hand) and all(_same(two[b], by_hand[b]) for b in R2.BLOCKS)
        shared = H.hci_transition_rdms(h, up, dn, w, 0, 1, g=gp)          # on the caller's open context: the same bytes
        assert _same(shared[0], one) and all(_same(shared[1][b], two[b]) for b in R2.BLOCKS)
        only = H.hci_transition_rdms(h, up, dn, w, 1, 0, blocks="ab")
        assert list(only[1]) == ["ab"] and _same(only[1]["ab"], np.asfortranarray(two["ab"].transpose(2, 3, 0, 1))) and _same(only[0], np.asfortranarray(one.T))
        with pytest.raises(ValueError):
            H.hci_transition_rdms(h, up, dn, w, 0, 2)
        # two Davidson eigenvectors: orthogonal, and a one-body transition matrix with a dominant singular value
        ovl = H.transition_overlap(h, one)
        sv, hole, part = H.natural_transition_orbitals(one)
        print("host layer: %d combinations, %d determinants, overlap %.3g, singular values %s" % (len(up), len(du), ovl, sv[:3]))
        assert abs(ovl) < 1e-8 and sv[0] > 1e-3 and np.all(np.diff(sv) <= 0)
        assert np.allclose(hole @ np.diag(sv) @ part.T, one, rtol=0, atol=1e-13)
        # two truncations of state 1 on lists of their own, paired through their union
        assert len(du) >= 160
        big = np.argsort(-np.abs(c0), kind="stable")
        a_ix, b_ix = np.sort(big[:90]), np.sort(big[40:160])
        uu, ud, ua, ub = H.union_expansion(du[a_ix], dd[a_ix], c0[a_ix], du[b_ix], dd[b_ix], c1[b_ix])
        assert len(uu) == 160 and np.count_nonzero(ua) <= 90 and np.count_nonzero(ub) <= 120 and np.array_equal(H.sort_dets(uu, ud), np.arange(160))
        dets = list(zip(uu.tolist(), ud.tolist()))
        got = gp.two_tdm(uu, ud, ua, ub)
        fails, worst, seen = R2.compare(TC.two_tdm(dets, ua.tolist(), ub.tolist(), h.norb), got)
        assert not fails and seen > 1000, fails[:4]
        assert not RC.compare(TC.one_tdm(dets, ua.tolist(), ub.tolist(), h.norb), gp.one_tdm(uu, ud, ua, ub))[0]
        with pytest.raises(ValueError):
            H.union_expansion(du[:3], dd[:3], c0[:3], du[[1, 1]], dd[[1, 1]], c0[:2])
    finally:
        gp.close()


def _deck_text(n_states=2):
    t = open(DECK).read().replace("1e-3  1e-7      1.e-4   2", "3e-2  1e-5      1.e-4   %d" % n_states).replace("eps_var_sched=2*2e-3", "eps_var_sched=2*6e-2")
    t = t.replace("f                                 dump_wf_var", "t                                 dump_wf_var")
    assert "3e-2  1e-5" in t and "2*6e-2" in t and "t                                 dump_wf_var" in t
    return t


def test_deck_with_transition_rdm(dev, tmp_path, monkeypatch):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    import sqmc_amd
    import copy
    monkeypatch.chdir(tmp_path)                                      # the deck dumps its wavefunction into the working directory
    deck = R.parse_hci_deck(_deck_text())
    buf, path = io.StringIO(), str(tmp_path / "tdm.npz")
    res = R.run_hci(deck, FCIDUMP, out=buf, transition_rdm_path=path)
    lines = buf.getvalue().splitlines()
    marks = ["Computing transition density matrices between the states of the variational wavefunction", "Transition density matrices of states   1 and   2:",
             "Transition density matrices written to " + path, "State   1:", "State   2:"]
    at = [lines.index(m) for m in marks]
    assert at == sorted(at) and len(set(at)) == len(at)
    i0 = at[1]
    assert lines[i0 + 1].startswith(" Overlap =") and lines[i0 + 2].startswith(" <i|H|j> from the density matrices =") and lines[i0 + 3].startswith(" <i|S^2|j> =")
    assert lines[i0 + 4].startswith(" Largest singular values of the one-body matrix =") and len(lines[i0 + 4].split("=")[1].split()) == 3
    rec = res["transition_rdm"]
    assert len(rec) == 1 and rec[0]["states"] == (1, 2) and len(res["states"]) == 2
    z = np.load(path)
    assert sorted(z.files) == ["aa_1_2", "ab_1_2", "bb_1_2", "one_1_2"] and z["ab_1_2"].shape == (26,) * 4 and z["one_1_2"].shape == (26, 26)
    with pytest.raises(FileExistsError):                             # a new file only
        R.run_hci(R.parse_hci_deck(_deck_text()), FCIDUMP, out=io.StringIO(), transition_rdm_path=path)
    # <1|H|2> of the deck against w1 . (H w2) from the resident plan of the dumped wavefunction, within the identity test's bound
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    up, dn, w, e = H.read_wf_var(H.wf_filename(3e-2), 2)
    w = np.asarray(w, float).reshape(len(up), -1)
    assert res["ndets"] == len(up) and 10 <= len(up) <= 600
    g = h.gpu()
    try:
        e_plan = _plan_element(sqmc_amd, H, g, np.asarray(up, np.uint64), np.asarray(dn, np.uint64), w[:, 0], w[:, 1])
    finally:
        g.close()
    du, dd, c0 = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
    _, _, c1 = H.time_symmetrized_to_dets(up, dn, w[:, 1], h.z)
    dets, bra, ket = list(zip(du.tolist(), dd.tolist())), c0.tolist(), c1.tolist()
    HH = PC.ChemH(FCIDUMP, [int(h.orb_order[i]) for i in range(1, h.norb + 1)])
    ovl = TC.overlap(bra, ket)
    _, b_chk = TC.energy(HH, TC.one_tdm(dets, bra, ket, h.norb), TC.two_tdm(dets, bra, ket, h.norb), ovl)
    want, bw, sa = TC.expectation(HH, dets, bra, ket)
    print("deck: %d combinations, %d determinants; <1|H|2> = %.3e (deck), %.3e (plan), %.3e (all pairs); bound %.3g"
          % (len(up), len(dets), rec[0]["h"], e_plan, want, 2 * b_chk + 2 * bw + 4 * len(dets) * RC.U * sa))
    # rdm_energy sums all norb^4 entries with numpy: norb^4 more roundings on the mass of its terms, as in the identity test
    _, sa_dev = _device_energy(HH, z["one_1_2"], {b: z[b + "_1_2"] for b in R2.BLOCKS}, ovl)
    assert abs(rec[0]["h"] - e_plan) <= 2 * b_chk + 2 * bw + 4 * len(dets) * RC.U * sa + (h.norb ** 4) * RC.U * sa_dev
    assert abs(rec[0]["overlap"]) < 1e-8 and abs(rec[0]["overlap"] - ovl) < 1e-14 and rec[0]["singular_values"][0] > 1e-3
    assert np.array_equal(z["one_1_2"], H.hci_transition_rdms(h, up, dn, w, 0, 1, blocks="ab")[0])
    # one state: the flag is refused with the reason, before any work
    with pytest.raises(SystemExit) as ex:
        R.run_hci(R.parse_hci_deck(_deck_text(1)), FCIDUMP, out=io.StringIO(), transition_rdm_path=str(tmp_path / "other.npz"))
    assert "--transition-rdm needs two states" in str(ex.value) and not os.path.exists(str(tmp_path / "other.npz"))
