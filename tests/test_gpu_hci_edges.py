"""The Heat-bath CI doors of the HIP library (sqmc_gpu_hci_connections, _slice, sqmc_gpu_hci_pt2) against tests/hci_checker.py,
which shares nothing with the library or the oracle, at the edges no deck reaches: unscreened rows of closed- and open-shell
sources, screened lists in merged and raw mode, the active-space masks under time-reversal symmetry, the tie conventions of the
three excitation classes, zero coefficients, eps above max_double, PT2 of tiny and of closed spaces in 1 to 64 slices; and,
anchored to those by additivity, source lists across the block (256) and scan-tile (2048) sizes, a 600-term run of one key in the
merge, the partition of the output by key slices, and an ordinary call after every refusal and every empty result.
The check functions are those of tests/test_hci_checker.py, which runs them on the CPU oracle.  All tolerances are the
checker's derived rounding bounds; every test prints its worst |delta| / bound."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import gpu_ctx_from_oracle, gpu_ctx_heg          # noqa: E402
from tests import hci_checker as HC                             # noqa: E402
from tests import test_hci_checker as TH                        # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


class GpuDoor:
    def __init__(self, sysm, which):
        import sqmc_amd
        sqmc_amd.set_device(0)
        if which.startswith("heg"):
            self.g = gpu_ctx_heg(sysm)
        else:
            self.g = gpu_ctx_from_oracle(sysm)
            r, s_, a, pi, pc = sysm.hb_tables()
            self.g.set_hb_tables(r, s_, a, pi, pc, sysm.s.max_double)

    def close(self):
        self.g.close()

    def set_active_space(self, *a):
        self.g.hci_set_active_space(*a)

    def connections(self, up, dn, coeffs, eps, diag_mode=0, slice=0, n_slices=1):
        return self.g.hci_connections(up, dn, coeffs, eps, diag_mode, slice, n_slices)

    def pt2(self, up, dn, coeffs, e_var, eps, n_slices=1):
        return self.g.hci_pt2(up, dn, coeffs, e_var, eps, n_slices)

    def element(self, a, b):
        f = lambda x: np.array([x], np.uint64)
        return float(self.g.hamiltonian_batch(f(a[0]), f(a[1]), f(b[0]), f(b[1]))[0])


@pytest.fixture
def door(request):
    made = []

    def make(which):
        sysm = request.getfixturevalue(which)
        d = GpuDoor(sysm, which)
        made.append(d)
        return d, TH.build_case(sysm, which), sysm
    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("which", TH.WHICH)
def test_unscreened_rows(door, which):
    d, c, _ = door(which)
    TH.check_unscreened_rows(d, c)


@pytest.mark.parametrize("which", ["c2_walk", "c2_hci", "heg14"])
def test_screened_lists_merged_and_raw(door, which):
    d, c, _ = door(which)
    TH.check_screened_lists(d, c, modes=(0, 2))


def test_active_space_modes_with_time_symmetry(door):
    d, c, _ = door("c2_hci")
    TH.check_active_space(d, c)


@pytest.mark.parametrize("which", ["c2_walk", "heg14", "heg57"])
def test_tie_conventions(door, which):
    """single: kept (chemistry.f90:6956); chemistry double: dropped (chemistry.f90:7042); HEG double: dropped (heg.f90:2608, 2629)"""
    d, c, sysm = door(which)
    TH.check_ties(d, c, sysm.hb_tables()[2] if c.chem else None)


@pytest.mark.parametrize("which", ["c2_walk", "c2_hci", "heg14"])
def test_zero_coefficients(door, which):
    d, c, _ = door(which)
    TH.check_zero_coefficients(d, c)
    u, dn = TH.arrays(c.sources)                       # an ordinary call after the empty results: the known-good answer
    exp = HC.connections(c.H, c.sources, c.coeffs, c.eps[1], 0, time_sym=c.ts, z=c.z)
    TH._clean("%s after the empty results" % which, exp, d.connections(u, dn, c.coeffs, c.eps[1], 0), 0)


@pytest.mark.parametrize("which", ["c2_walk", "c2_hci"])
def test_eps_above_max_double(door, which):
    d, c, sysm = door(which)
    TH.check_eps_above_max_double(d, c, sysm.s.max_double)


@pytest.mark.parametrize("which", ["c2_walk", "c2_hci", "heg14"])
def test_pt2_against_brute_force(door, which):
    """n_var = 1, a small space, a space closed under the screened generator (delta_e exactly 0.0) and one whose outside
    determinants hold both the smallest and the largest key in sight, each in 1, 2, 5 and 64 slices: delta_e within the
    checker's bound every time, n_connections the checker's count of visited determinants and the same for every slice count"""
    d, c, _ = door(which)
    for name, var, co, eps, zero in TH.pt2_spaces(c):
        if var is None:
            var, co = TH.extreme_key_space(c)
            eps = c.eps[1]
        order = sorted(range(len(var)), key=lambda k: var[k])
        var, co = [var[k] for k in order], [co[k] for k in order]
        print(name, end=": ")
        TH.check_pt2(d, c, var, co, TH.e_var_of(c, var, co), eps, slices=(1, 2, 5, 64), want_zero=zero)


# ---------------------------------------------------------------------------------------------- anchored by additivity
_BFS = {}
N_BFS = 2049


def _bfs_sources(d, c, n):
    """the first n of 2049 sources found by breadth-first connection from HF through the door itself (which determinants they
    are does not matter to an additivity check), in sorted order; coefficients of mixed sign between 1 and 1e-2 that depend on
    the position alone, so that every list is a prefix of the longest"""
    if c.which not in _BFS:
        have, eps = [c.sources[0]], 1e-3
        while len(have) < N_BFS:
            u, dn = TH.arrays(have[:64])
            cu, cd, _, _ = d.connections(u, dn, np.ones(len(u)), eps)
            have = sorted(set(have) | set(zip(cu.tolist(), cd.tolist())))
            eps *= 0.5
            assert eps > 1e-9
        k = np.arange(N_BFS)
        _BFS[c.which] = (have[:N_BFS], 10.0 ** (-2.0 * (k % 97) / 96.0) * np.where(k % 3 == 1, -1.0, 1.0))
    src, co = _BFS[c.which]
    return src[:n], co[:n].copy()


def _chunk_eps(c, src, co):
    """HEG14: a threshold from pick_eps over the paths of the first 256 sources (the ones whose chunks go to the checker), which
    keeps nine tenths of them; C2 (no checker in this test, rows are long): 1e-4"""
    if c.which != "heg14":
        return 1e-4
    m = min(len(src), 256)
    vals = HC.screen_values(c.H, src[:m], co[:m].tolist())
    return HC.pick_eps(vals, TH._k_for(vals, (9 * len(vals)) // 10))


SIZES = [1, 255, 256, 257, 2047, 2048, 2049]


@pytest.mark.parametrize("which,n_ref", [(w, n) for w in ("heg14", "c2_walk") for n in SIZES])
def test_whole_list_equals_its_chunks(door, which, n_ref):
    """one call on the whole list against calls on chunks of 7 sources merged on the host in source order: identical sets,
    e_mix_den exact, sums within n_contrib 2^-53 sum|terms| per determinant (n_contrib and sum|terms| from the raw mode of the
    same chunks); on HEG14 every chunk of the first 256 sources is checked against the checker, none with a borderline path"""
    d, c, _ = door(which)
    src, co = _bfs_sources(d, c, n_ref)
    eps = _chunk_eps(c, *_bfs_sources(d, c, N_BFS)) if n_ref > 1 else _chunk_eps(c, src, co)
    u, dn = TH.arrays(src)
    wu, wd, wn, we = d.connections(u, dn, co, eps)
    num, den, cnt, sab = {}, {}, {}, {}
    total, worst_chunk, checked = 0, 0.0, 0
    for a in range(0, n_ref, 7):
        b = min(a + 7, n_ref)
        cu, cd, cn, ce = d.connections(u[a:b], dn[a:b], co[a:b], eps)
        if which == "heg14" and a < 256:
            exp = HC.connections(c.H, src[a:b], co[a:b].tolist(), eps, 0)
            assert not exp.borderline, (a, exp.borderline[:3])
            fails, w = HC.compare(exp, cu, cd, cn, ce)
            assert not fails, (a, fails[:4])
            worst_chunk, checked = max(worst_chunk, w), checked + 1
        ru, rd, rn, _ = d.connections(u[a:b], dn[a:b], co[a:b], eps, 2)
        total += len(ru)
        for k, x in zip(zip(ru.tolist(), rd.tolist()), rn.tolist()):
            cnt[k] = cnt.get(k, 0) + 1; sab[k] = sab.get(k, 0.0) + abs(x)
        for k, x, y in zip(zip(cu.tolist(), cd.tolist()), cn.tolist(), ce.tolist()):
            if k in num:
                num[k] = num[k] + x; den[k] = den[k] + y
            else:
                num[k], den[k] = x, y
    ks = sorted(num)
    assert [k[0] for k in ks] == wu.tolist() and [k[1] for k in ks] == wd.tolist()
    assert [den[k] for k in ks] == we.tolist()
    if which == "heg14":
        assert checked == (min(n_ref, 256) + 6) // 7
    worst, at = 0.0, None
    for k, x in zip(ks, wn.tolist()):
        b = cnt[k] * U * sab[k]
        assert abs(x - num[k]) <= b, (k, x, num[k], b)
        if b > 0 and abs(x - num[k]) / b > worst:
            worst, at = abs(x - num[k]) / b, k
    print("%s n_ref %d eps %.3g: %d raw connections, %d determinants, worst |delta| / bound = %.3g%s (%d chunks against the checker: %.3g)" % (
        which, n_ref, eps, total, len(ks), worst, " at (%#x, %#x), %d terms" % (at + (cnt[at],)) if at else "", checked, worst_chunk))
    if n_ref > 1:
        assert total > 1024
    if n_ref > 2000 and which == "c2_walk":              # the large-n sort path (HEG14 rows are too short to reach it)
        assert total > 1 << 20


def test_long_run_of_one_key(door):
    """600 sources that all reach one determinant D (HF), D itself not in the list: the merge adds about 600 terms into D's sum"""
    d, c, _ = door("c2_walk")
    D = c.sources[0]
    row = sorted((p for p in HC.raw_paths(c.H, D) if not p.noise and abs(p.raw) > 1e-6), key=lambda p: p.det)[:600]
    assert len(row) == 600
    src = [p.det for p in row]
    co = [(-1.0 if k % 2 else 1.0) * (0.5 + (k % 7) / 10.0) for k in range(600)]
    els = [c.H.element(s[0], s[1], D[0], D[1]) for s in src]
    terms = [e[0] * x for e, x in zip(els, co)]
    want = math.fsum(terms)
    bound = math.fsum((HC.PC.rounding_bound(e[1], e[2]) + 4 * U * abs(e[0])) * abs(x) for e, x in zip(els, co)) + 600 * U * math.fsum(abs(t) for t in terms)
    u, dn = TH.arrays(src)
    gu, gd, gn, ge = d.connections(u, dn, co, 1e-9)
    k = list(zip(gu.tolist(), gd.tolist())).index(D)
    print("run of 600: D's sum %r against %r, |delta| / bound = %.3g" % (gn[k], want, abs(gn[k] - want) / bound))
    assert abs(gn[k] - want) <= bound and ge[k] == 0.0


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_slices_partition_the_output(door, which):
    """40 sources.  HEG14: the 40-determinant list of the PT2 test, the unsliced output anchored to the checker; C2: 40 sources by
    breadth-first connection (a C2 row costs the checker 2 s), the slices anchored to the unsliced call alone"""
    d, c, _ = door(which)
    if which == "heg14":
        src, co, eps = TH.long_list(c, 40)
    else:
        src, co = _bfs_sources(d, c, 40)
        eps = 1e-4
    assert len(src) == 40
    u, dn = TH.arrays(src)
    whole = d.connections(u, dn, co, eps)
    if which == "heg14":
        exp = HC.connections(c.H, src, co, eps, 0)
        TH._clean("%s unsliced" % which, exp, whole, 0)
    for ns in (2, 3, 7, 64, 4096):
        parts, empty = [], 0
        for s in range(ns):
            got = d.connections(u, dn, co, eps, 0, s, ns)
            empty += len(got[0]) == 0
            for a, b in zip(got[0].tolist(), got[1].tolist()):
                assert HC.slice_index((a, b), c.norb, c.nup, c.ndn, ns) == s, (ns, s, hex(a), hex(b))
            parts.append(got)
        for col in range(4):                                  # in slice order: exactly the unsliced arrays, bit for bit
            assert np.array_equal(np.concatenate([p[col] for p in parts]), whole[col]), (ns, col)
        print("%s: %d slices, %d empty" % (which, ns, empty))
        assert ns < 64 or empty > 0
    for bad in ((2, 2), (-1, 2), (0, 0), (5, 3)):
        with pytest.raises(Exception):
            d.connections(u, dn, co, eps, 0, bad[0], bad[1])
        again = d.connections(u, dn, co, eps)           # the next call works
        assert all(np.array_equal(x, y) for x, y in zip(again, whole))
    raw = d.connections(u, dn, co, eps, 2)
    for ns in (3, 64):                                        # raw mode: the slices partition the generation list too
        n = sum(len(d.connections(u, dn, co, eps, 2, s, ns)[0]) for s in range(ns))
        assert n == len(raw[0])
    again = d.connections(u, dn, co, eps)
    assert all(np.array_equal(x, y) for x, y in zip(again, whole))
