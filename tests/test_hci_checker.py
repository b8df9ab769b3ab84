"""tests/hci_checker.py against the CPU oracle's HCI side (important_connected, hci_pt2), on the inputs that
tests/test_gpu_hci_edges.py hands to the HIP doors: the same check functions run here with the oracle behind the `door` and
there with the library, so that a failure there can be told from a failure of the checker or of the inputs.  Also: every
doctored output is rejected by the comparison, and no case that is not about ties has a path on its threshold.

Checker wall time on one CPU core: a C2 row (10 692 pairs) takes 1.2 to 2.0 s, so the 8-source C2 lists (the fewest the
lists may have) cost 10 to 16 s per system and the four further rows of the 12-determinant PT2 space 5 to 8 s, once per session
(rows are cached in hci_checker); a HEG14 row 0.1 s (the 40-determinant list 4 s), a HEG57 row 0.9 s (8 sources 7 s).
Each test prints its own."""
import math
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hci_checker as HC               # noqa: E402
from tests import test_proposal_unbiased as TU    # noqa: E402

WHICH = ["c2_walk", "c2_hci", "heg14", "heg57"]
N_SOURCES = {"c2_walk": 8, "c2_hci": 8, "heg14": 16, "heg57": 8}
_CASES = {}


# ---------------------------------------------------------------------------------------------- the inputs
class Case:
    pass


def build_case(sysm, which):
    """sources: HF, then the determinants HF's strongest paths reach, among them an open-shell one, a closed-shell one other than
    HF and (time symmetry) one that is reached as a swapped representative; coefficients of mixed sign from 0.1 down to 1e-3;
    three thresholds from pick_eps: nearly everything, half, a handful"""
    if which in _CASES:
        return _CASES[which]
    t0 = time.time()
    c = Case()
    c.which, c.chem = which, which.startswith("c2")
    c.ts, c.z = which == "c2_hci", 1
    c.H = TU.chem_checker(sysm) if c.chem else TU.heg_checker(sysm)
    c.norb, c.nup, c.ndn = c.H.norb, sysm.nup, sysm.ndn
    hf = (sysm.hf_up, sysm.hf_dn)
    row = sorted((p for p in HC.raw_paths(c.H, hf, c.ts, c.z) if not p.noise), key=lambda p: (-abs(p.raw), p.det))
    open_ = next(p.det for p in row if p.det[0] != p.det[1])
    closed = next((p.det for p in row if p.det[0] == p.det[1]), None)
    if closed is None:                      # no double of the HEG's HF keeps the two strings equal: both strings take the open one's
        closed = (max(open_),) * 2
    c.rows = [("hf", hf), ("open_shell", open_), ("closed_shell", closed)]
    if c.ts:
        c.rows.append(("swapped", next(p.det for p in row if p.det != p.new)))
    src = [hf] + [d for _, d in c.rows[1:]]
    for p in row:
        if len(src) >= N_SOURCES[which]:
            break
        if p.det not in src:
            src.append(p.det)
    c.sources = src
    n = len(src)
    c.coeffs = [float(x) * (-1.0 if k % 3 == 1 else 1.0) for k, x in enumerate(np.geomspace(0.1, 1e-3, n))]
    vals = HC.screen_values(c.H, src, c.coeffs, c.ts, c.z)
    nv = len({abs(v) for v in vals})
    c.n_paths = len(vals)
    c.eps = [HC.pick_eps(vals, min(_k_for(vals, len(vals) - 3), nv - 1)), HC.pick_eps(vals, _k_for(vals, len(vals) // 2)), HC.pick_eps(vals, _k_for(vals, 12))]
    c.row_eps = {name: 0.5 * min(abs(p.raw) for p in HC.raw_paths(c.H, d, c.ts, c.z) if not p.noise) for name, d in c.rows}
    c.checker_seconds = time.time() - t0
    print("%s: %d sources, %d distinct |H c|, eps %s; checker rows %.1f s" % (which, n, nv, ["%.3g" % e for e in c.eps], c.checker_seconds))
    _CASES[which] = c
    return c


def _k_for(vals, count):
    """the number of distinct values, from the largest down, that at least `count` paths carry (many HEG paths share one value)"""
    import collections
    count_of = collections.Counter(abs(x) for x in vals)
    seen, k = 0, 0
    for v in sorted(count_of, reverse=True):
        k += 1
        seen += count_of[v]
        if seen >= count:
            break
    return k


def arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


# ---------------------------------------------------------------------------------------------- the oracle behind the door
class OracleDoor:
    """the generator's door as the library offers it (merged and sorted, or raw with the source index), made of the oracle's
    important_connected: left-to-right sums in source order, a zero coefficient gives nothing"""

    def __init__(self, oracle, sysm):
        self.O, self.sysm = oracle, sysm
        sysm.setup_hb()

    def set_active_space(self, *a):
        self.sysm.set_active_space(*a)

    def connections(self, up, dn, coeffs, eps, diag_mode=0):
        ru, rd, rn, rs, first = [], [], [], [], []
        for i, (u, d, c) in enumerate(zip(np.asarray(up).tolist(), np.asarray(dn).tolist(), np.asarray(coeffs, float).tolist())):
            if c == 0.0:
                continue
            xu, xd, xe = self.sysm.important_connected(u, d, eps / abs(c))
            xe = xe * c
            if diag_mode == 1:
                xe[0] = self.sysm.ham(u, d, u, d) * c
            ru += xu.tolist(); rd += xd.tolist(); rn += xe.tolist(); rs += [i] * len(xu); first += [c] + [0.0] * (len(xu) - 1)
        if diag_mode == 2:
            return np.array(ru, np.uint64), np.array(rd, np.uint64), np.array(rn), np.array(rs, float)
        num, den = {}, {}
        for u, d, x, y in zip(ru, rd, rn, first):
            if (u, d) in num:
                num[(u, d)] = num[(u, d)] + x; den[(u, d)] = den[(u, d)] + y
            else:
                num[(u, d)], den[(u, d)] = x, y
        ks = sorted(num)
        a, b = arrays(ks)
        return a, b, np.array([num[k] for k in ks]), np.array([den[k] for k in ks])

    def pt2(self, up, dn, coeffs, e_var, eps, n_slices=1):
        d, _ = self.O.hci_pt2(self.sysm, up, dn, coeffs, e_var, eps)
        return d, len(self.connections(up, dn, coeffs, eps)[0])

    def ham(self, det):
        return self.sysm.ham(det[0], det[1], det[0], det[1])

    def element(self, a, b):
        return self.sysm.ham(a[0], a[1], b[0], b[1])


# ---------------------------------------------------------------------------------------------- the checks (door: oracle or library)
def _clean(tag, exp, got, mode):
    fails, worst = HC.compare(exp, *got, diag_mode=mode)
    print("%-44s mode %d: %5d determinants, %3d optional, worst |delta| / bound = %.3g%s" % (
        tag, mode, len(exp.merged), len(exp.optional), worst, " at (%#x, %#x)" % exp.worst_at if exp.worst_at else ""))
    assert not fails, (tag, mode, fails[:6])
    return worst


def check_unscreened_rows(door, c):
    """one source, c = 1, eps below the smallest non-zero |H| of its row: the non-zero row plus the self slot, each num within
    its bound, den = c on the self slot and 0 elsewhere; the self slot exactly 0.0 in mode 0 and H_ii within bound in mode 1"""
    for name, det in c.rows:
        u, d = arrays([det])
        for mode in (0, 1):
            exp = HC.connections(c.H, [det], [1.0], c.row_eps[name], mode, time_sym=c.ts, z=c.z)
            assert not exp.borderline
            got = door.connections(u, d, [1.0], c.row_eps[name], mode)
            _clean("%s row %s" % (c.which, name), exp, got, mode)
            k = list(zip(got[0].tolist(), got[1].tolist())).index(det)
            assert got[3][k] == 1.0 and np.count_nonzero(got[3]) == 1
            if mode == 0 and det in exp.exact_zero:
                assert got[2][k] == 0.0


def check_screened_lists(door, c, modes=(0, 2)):
    u, d = arrays(c.sources)
    for eps in c.eps:
        for mode in modes:
            exp = HC.connections(c.H, c.sources, c.coeffs, eps, mode, time_sym=c.ts, z=c.z)
            assert not exp.borderline, exp.borderline[:3]
            _clean("%s list eps %.3g" % (c.which, eps), exp, door.connections(u, d, c.coeffs, eps, mode), mode)
    kept = [len(HC.connections(c.H, c.sources, c.coeffs, e, 0, time_sym=c.ts, z=c.z).raw) for e in c.eps]
    n = len(c.sources)
    assert kept[0] - n > 0.9 * c.n_paths and 0.3 * c.n_paths < kept[1] - n < 0.7 * c.n_paths and 6 <= kept[2] - n <= 40 + 0.02 * c.n_paths, (kept, c.n_paths)


def active_space_of(c):
    """the lowest orbital of either spin frozen, the last 8 orbitals virtual (the masks of test_hci_connections_active_space_masks)"""
    virt = ((1 << c.norb) - 1) ^ ((1 << (c.norb - 8)) - 1)
    return 1, 1, virt, virt


def check_active_space(door, c):
    u, d = arrays(c.sources)
    eps = c.eps[1]
    sizes = {}
    try:
        for mode in (0, 1, 2):
            door.set_active_space(*active_space_of(c), mode)
            exp = HC.connections(c.H, c.sources, c.coeffs, eps, 0, active_space=active_space_of(c) + (mode,), time_sym=c.ts, z=c.z)
            assert not exp.borderline
            _clean("%s active-space mode %d" % (c.which, mode), exp, door.connections(u, d, c.coeffs, eps, 0), 0)
            sizes[mode] = len(exp.raw)
    finally:
        door.set_active_space(0, 0, 0, 0, 0)
    n = len(c.sources)
    assert sizes[1] > n and sizes[2] > n and sizes[1] + sizes[2] == sizes[0] + n, sizes


def check_zero_coefficients(door, c):
    """A source with c == 0 is never handed to the generator (semistoch.f90:1762, 1798, 1854, 1891): nothing comes from it, its
    own slot included; it appears only where another source reaches it, with e_mix_den = 0.  First, middle and last position, alone
    and among others."""
    src = c.sources[:5]
    u, d = arrays(src)
    eps = c.eps[1]
    got = door.connections(u[:1], d[:1], [0.0], eps, 0)
    assert len(got[0]) == 0
    for zeros in ([0], [2], [4], [0, 2, 4], [0, 1, 2, 3, 4]):
        co = [0.0 if k in zeros else x for k, x in enumerate(c.coeffs[:5])]
        for mode in (0, 2):
            exp = HC.connections(c.H, src, co, eps, mode, time_sym=c.ts, z=c.z)
            assert not exp.borderline
            _clean("%s zero coefficient at %s" % (c.which, zeros), exp, door.connections(u, d, co, eps, mode), mode)


def check_eps_above_max_double(door, c, max_double):
    """eps / |c| above the largest double-excitation element: the doubles loop is skipped (chemistry.f90:6995), singles and the
    self slots remain"""
    src, co = c.sources[:4], [1.0, -1.0, 0.5, -0.5]
    u, d = arrays(src)
    eps = 1.0000001 * max_double
    exp = HC.connections(c.H, src, co, eps, 0, time_sym=c.ts, z=c.z)
    assert not exp.borderline
    for s in src:
        assert all(p.cls == HC.SINGLE for p in HC.raw_paths(c.H, s, c.ts, c.z) if abs(p.raw) >= eps)
    _clean("%s eps above max_double" % c.which, exp, door.connections(u, d, co, eps, 0), 0)
    got = door.connections(u, d, co, 0.5 * eps, 0)          # |c| = 0.5: eps / |c| = eps again for those two; for |c| = 1 the doubles are back
    exp = HC.connections(c.H, src, co, 0.5 * eps, 0, time_sym=c.ts, z=c.z)
    assert not exp.borderline
    _clean("%s eps above max_double for half of the list" % c.which, exp, got, 0)


def check_ties(door, c, stored_abs=None):
    """Which side of |H c| == eps is kept, per class, as the reference has it; c = +1 and c = -1.
       single            kept      chemistry.f90:6956   if (abs(matrix_element)<eps) cycle
       chemistry double  dropped   chemistry.f90:7042   if (dtm_hb(...)%absH<=eps) exit
       HEG double        dropped   heg.f90:2608, 2629   exit at absH <= eps
    The threshold is the door's own element of the pair (for a chemistry double the stored heat-bath entry, stored_abs), only so
    that the tie is exact; one ulp below it everything of that size is kept, one ulp above it dropped."""
    hf = c.sources[0]
    paths = [p for p in HC.raw_paths(c.H, hf, c.ts, c.z) if not p.noise and p.det == p.new]
    by_det = {}
    for p in HC.raw_paths(c.H, hf, c.ts, c.z):
        by_det.setdefault(p.det, []).append(p)
    u, d = arrays([hf])
    done = set()
    for p in sorted(paths, key=lambda p: (-abs(p.raw), p.det)):
        if p.cls in done or len(by_det[p.det]) != 1:
            continue
        h = abs(door.element(hf, p.new))
        if p.cls == HC.DOUBLE:
            k = int(np.argmin(np.abs(stored_abs - abs(p.raw))))
            h = float(stored_abs[k])
        assert abs(h - abs(p.raw)) <= PC.rounding_bound(p.n, p.s)
        done.add(p.cls)
        for sign in (1.0, -1.0):
            exp = HC.connections(c.H, [hf], [sign], h, 0, time_sym=c.ts, z=c.z)
            assert any(b[1] == p.det for b in exp.borderline)            # the checker sees the tie and leaves it open
            here = lambda e: p.det in set(zip(*[x.tolist() for x in door.connections(u, d, [sign], e, 0)[:2]]))
            assert here(math.nextafter(h, 0.0)), (p.cls, sign, "dropped below the tie")
            assert not here(math.nextafter(h, math.inf)), (p.cls, sign, "kept above the tie")
            assert here(h) == HC.KEEPS_TIE[p.cls], (p.cls, sign, "wrong side of the tie")
    assert done == ({HC.SINGLE, HC.DOUBLE} if c.chem else {HC.HEG}), done


def check_pt2(door, c, var, coeffs, e_var, eps, slices=(1,), want_zero=False):
    u, d = arrays(var)
    want, n_out, n_visited, bound, borderline = HC.pt2(c.H, var, coeffs, e_var, eps, c.ts, c.z)
    assert not borderline
    worst = 0.0
    for ns in slices:
        got, n = door.pt2(u, d, coeffs, e_var, eps, ns)
        assert n == n_visited, (ns, n, n_visited)
        if want_zero:
            assert got == 0.0 and want == 0.0 and n_out == 0
        else:
            assert abs(got - want) <= bound, (ns, got, want, bound)
            worst = max(worst, abs(got - want) / bound)
    print("%s PT2: %d in the space, %d outside, delta_e %.12g, worst |delta| / bound = %.3g over n_slices %s" % (
        c.which, len(var), n_out, want, worst, list(slices)))
    return want


def e_var_of(c, var, coeffs):
    """a variational energy below every diagonal element in sight: the lowest diagonal of the space minus 0.1"""
    return min(HC.diagonal(c.H, v, c.ts, c.z)[0] for v in var) - 0.1


N_PT2 = {"c2_walk": 12, "c2_hci": 12, "heg14": 40}


def long_list(c, n):
    """c.sources continued with the determinants HF's next strongest paths reach, n in all; coefficients of mixed sign from 0.1
    down to 1e-3; a threshold from pick_eps that keeps about half of the list's paths"""
    key = ("long", n)
    if not hasattr(c, "_long"):
        c._long = {}
    if key not in c._long:
        src = list(c.sources)
        row = sorted((p for p in HC.raw_paths(c.H, src[0], c.ts, c.z) if not p.noise), key=lambda p: (-abs(p.raw), p.det))
        for p in row:
            if len(src) >= n:
                break
            if p.det not in src:
                src.append(p.det)
        assert len(src) == n
        co = [float(x) * (-1.0 if k % 3 == 1 else 1.0) for k, x in enumerate(np.geomspace(0.1, 1e-3, n))]
        vals = HC.screen_values(c.H, src, co, c.ts, c.z)
        c._long[key] = (src, co, HC.pick_eps(vals, _k_for(vals, len(vals) // 2)))
    return c._long[key]


def pt2_spaces(c):
    """[(name, determinants, coefficients, eps, expect delta_e == 0)]: HF alone, the 12-determinant C2 / 40-determinant HEG14
    space, on HEG14 a space closed under the screened generator, and one whose outside determinants hold the extreme keys.

    The closed space is weaker than 'a first-order space plus every connection found at that eps' with every coefficient live:
    only HF and two first-order determinants keep coefficients that let them generate; all the others get 1e-7, so that eps / |c|
    is above every element and they generate nothing.  With two live levels the closure of HEG14 already holds 3169 determinants
    (300 s of checker rows), and a C2 closure costs 2 s per determinant; what the case pins all the same is delta_e == 0.0
    exactly, through every slice count, and n_connections."""
    out = [("hf alone", c.sources[:1], [1.0], c.eps[1], False)]
    n = N_PT2[c.which]
    src, co, eps = long_list(c, n)
    out.append(("%d determinants" % n, src, co, eps, False))
    if c.which == "heg14":
        # closed under the screened generator: HF (c = 1) and what it reaches at eps; two of those keep a coefficient (+-0.99) that
        # lets them generate at eps, and what they reach is added; every other coefficient (1e-7) puts eps / |c| above every
        # element, so those determinants generate nothing
        hf = c.sources[0]
        eps = HC.pick_eps(HC.screen_values(c.H, [hf], [1.0]), 1)
        first = sorted(HC.connections(c.H, [hf], [1.0], eps).merged)
        strong = [v for v in first if v != hf][:2]
        co1 = [1.0 if v == hf else (0.99 if v == strong[0] else -0.99) if v in strong else 1e-7 for v in first]
        second = sorted(set(HC.connections(c.H, [hf] + strong, [1.0, 0.99, -0.99], eps).merged) - set(first))
        assert len(first) > 4 and second
        out.append(("closed space", first + second, co1 + [1e-7 if k % 2 else -1e-7 for k in range(len(second))], eps, True))
    out.append(("extreme keys", None, None, None, False))
    return out


def extreme_key_space(c):
    """a two-determinant space whose connections include the determinant with the smallest key (the lowest orbitals of both
    strings) and one with the largest key in sight (orbital norb - 1 in the up string): HF is the smallest determinant there is,
    so the space is {a double of HF, a determinant holding orbital norb - 1} and HF is outside it"""
    hf = c.sources[0]
    row = [p for p in HC.raw_paths(c.H, hf, c.ts, c.z) if not p.noise]
    top = 1 << (c.norb - 1)
    a = max((p for p in row if not p.det[0] & top), key=lambda p: (abs(p.raw), p.det)).det
    b = max((p for p in row if p.det[0] & top), key=lambda p: (abs(p.raw), p.det)).det
    return sorted([a, b]), [0.7, -0.6]


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("which", WHICH)
def test_checker_matches_oracle_connections(request, oracle, which):
    sysm = request.getfixturevalue(which)
    c = build_case(sysm, which)
    door = OracleDoor(oracle, sysm)
    t0 = time.time()
    check_unscreened_rows(door, c)
    check_screened_lists(door, c)
    check_zero_coefficients(door, c)
    if c.chem:
        check_eps_above_max_double(door, c, sysm.s.max_double)
    print("%s: checker rows %.1f s, checks %.1f s" % (which, c.checker_seconds, time.time() - t0))


def test_checker_matches_oracle_active_space(request, oracle):
    sysm = request.getfixturevalue("c2_hci")
    check_active_space(OracleDoor(oracle, sysm), build_case(sysm, "c2_hci"))


@pytest.mark.parametrize("which", ["c2_walk", "heg14", "heg57"])
def test_tie_conventions_of_the_oracle(request, oracle, which):
    sysm = request.getfixturevalue(which)
    stored = sysm.hb_tables()[2] if which.startswith("c2") else None
    check_ties(OracleDoor(oracle, sysm), build_case(sysm, which), stored)


@pytest.mark.parametrize("which", ["c2_walk", "c2_hci", "heg14"])
def test_checker_matches_oracle_pt2(request, oracle, which):
    sysm = request.getfixturevalue(which)
    c = build_case(sysm, which)
    door = OracleDoor(oracle, sysm)
    for name, var, co, eps, zero in pt2_spaces(c):
        if var is None:
            var, co = extreme_key_space(c)
            eps = c.eps[1]
            keys = [HC.det_key(v, c.norb, c.ndn) for v in var]
            con = HC.connections(c.H, var, co, eps, time_sym=c.ts, z=c.z)
            outside = [HC.det_key(k, c.norb, c.ndn) for k in con.merged if k not in var]
            assert min(outside) < min(keys) and max(outside) > max(keys)
        order = sorted(range(len(var)), key=lambda k: var[k])
        var, co = [var[k] for k in order], [co[k] for k in order]
        print(name, end=": ")
        check_pt2(door, c, var, co, e_var_of(c, var, co), eps, want_zero=zero)


def _doctored(c):
    """a correct result of the HEG14 list at the middle threshold, as the door returns it, and the checker's expectation"""
    eps = c.eps[1]
    exp = HC.connections(c.H, c.sources, c.coeffs, eps, 0)
    ks = sorted(exp.merged)
    good = [[k[0] for k in ks], [k[1] for k in ks], [exp.merged[k][0] for k in ks], [exp.merged[k][1] for k in ks]]
    return eps, exp, ks, good


def test_doctored_outputs_are_rejected(request):
    """every doctoring of a correct result must fail compare(): the comparison has the power the GPU tests rely on"""
    sysm = request.getfixturevalue("heg14")
    c = build_case(sysm, "heg14")
    eps, exp, ks, good = _doctored(c)
    assert HC.compare(exp, *good)[0] == []
    copy = lambda: [list(x) for x in good]
    weakest = min((k for k in ks if k not in c.sources and len(exp.parts[k]) == 1), key=lambda k: abs(exp.merged[k][0]))
    strongest = max((k for k in ks if k not in c.sources), key=lambda k: abs(exp.merged[k][0]))
    cases = {}
    g = copy(); j = ks.index(weakest)
    for col in g: del col[j]
    cases["one weak connection dropped"] = (exp, g, 0)
    below = max((abs(p.raw * co), p.det, p.value * co) for s, co in zip(c.sources, c.coeffs) for p in HC.raw_paths(c.H, s)
                if not p.noise and abs(p.raw * co) < eps and p.det not in exp.merged)
    g = copy(); j = sum(1 for k in ks if k < below[1])
    for col, v in zip(g, (below[1][0], below[1][1], below[2], 0.0)): col.insert(j, v)
    cases["one connection just below the threshold added"] = (exp, g, 0)
    g = copy(); g[2][ks.index(strongest)] *= -1.0
    cases["one sign flipped"] = (exp, g, 0)
    multi = next(k for k in ks if len(exp.parts[k]) > 1)
    g = copy(); j = ks.index(multi); first = exp.parts[multi][0][0]
    g[2][j] -= first
    for col, v in zip(g, (multi[0], multi[1], first, 0.0)): col.insert(j, v)
    cases["one duplicate left unmerged"] = (exp, g, 0)
    g = copy(); src_k = 3
    for p in HC.raw_paths(c.H, c.sources[src_k]):
        if p.det in exp.merged and not p.noise and abs(p.raw * c.coeffs[src_k]) > eps:
            g[2][ks.index(p.det)] += p.value * c.coeffs[src_k]
    cases["one source's contribution added twice"] = (exp, g, 0)
    neg = HC.connections(c.H, c.sources, c.coeffs, eps, 0, threshold=lambda co: eps / co)
    kn = sorted(neg.merged)
    assert len(kn) > len(ks)
    cases["c instead of |c| in the screen"] = (exp, [[k[0] for k in kn], [k[1] for k in kn], [neg.merged[k][0] for k in kn], [neg.merged[k][1] for k in kn]], 0)
    # slices: the determinant with the largest key of slice 0 of 2 handed over to slice 1
    sl = lambda s: (lambda det: HC.slice_index(det, c.norb, c.nup, c.ndn, 2) == s)
    e0, e1 = HC.connections(c.H, c.sources, c.coeffs, eps, 0, slice_of=sl(0)), HC.connections(c.H, c.sources, c.coeffs, eps, 0, slice_of=sl(1))
    assert e0.merged and e1.merged and len(e0.merged) + len(e1.merged) == len(ks)
    k0, k1 = sorted(e0.merged), sorted(e1.merged)
    assert k0 + k1 == ks
    mk = lambda e, kk: [[k[0] for k in kk], [k[1] for k in kk], [e[k][0] for k in kk], [e[k][1] for k in kk]]
    assert HC.compare(e0, *mk(e0.merged, k0))[0] == [] and HC.compare(e1, *mk(e1.merged, k1))[0] == []
    both = dict(e0.merged); both.update(e1.merged)
    cases["one determinant moved to the next slice: the slice it left"] = (e0, mk(both, k0[:-1]), 0)
    cases["one determinant moved to the next slice: the slice it joined"] = (e1, mk(both, k0[-1:] + k1), 0)
    # diag_mode 1: 0 instead of H_ii in a self slot
    exp1 = HC.connections(c.H, c.sources, c.coeffs, eps, 1)
    g = mk(exp1.merged, sorted(exp1.merged))
    assert HC.compare(exp1, *g, diag_mode=1)[0] == []
    lonely = next(s for s in c.sources if len(exp1.parts[s]) == 1)
    g[2][sorted(exp1.merged).index(lonely)] = 0.0
    cases["0 instead of H_ii in a diag_mode 1 self slot"] = (exp1, g, 1)
    # raw mode: a connection credited to the neighbouring source
    exp2 = HC.connections(c.H, c.sources, c.coeffs, eps, 2)
    g = [[r[0][0] for r in exp2.raw], [r[0][1] for r in exp2.raw], [r[2] for r in exp2.raw], [float(r[1]) for r in exp2.raw]]
    assert HC.compare(exp2, *g, diag_mode=2)[0] == []
    j = next(k for k in range(1, len(exp2.raw)) if exp2.raw[k][1] == 1 and exp2.raw[k - 1][1] == 1)
    g[3][j] = 2.0
    cases["raw mode: a connection credited to another source"] = (exp2, g, 2)
    for name, (e, g, mode) in cases.items():
        fails, _ = HC.compare(e, *g, diag_mode=mode)
        print("%-66s -> %s" % (name, fails[0] if fails else "ACCEPTED"))
        assert fails, name


def test_pick_eps_and_slice_index():
    assert HC.pick_eps([1.0, 0.25, 0.25 * (1 + 1e-9), 0.01], 1) == math.sqrt(0.25 * (1 + 1e-9))
    assert HC.pick_eps([1.0, 0.25, 0.25 * (1 + 1e-9), 0.01], 2) == math.sqrt(0.25 * 0.01)
    norb, nup, ndn = 26, 4, 4
    assert HC.det_key((0xf, 0xf), norb, ndn) == 0 and HC.colex_rank(0b10111) == 1
    space = HC.key_space(norb, nup, ndn)
    assert space == 1 << 28
    last = (0xf << 22, 0xf << 22)
    assert HC.det_key(last, norb, ndn) == math.comb(26, 4) ** 2 - 1
    for ns in (2, 3, 7, 64, 4096):
        assert HC.slice_index((0xf, 0xf), norb, nup, ndn, ns) == 0
        s = HC.slice_index(last, norb, nup, ndn, ns)
        k = HC.det_key(last, norb, ndn)
        assert (space * s) // ns <= k and (s == ns - 1 or k < (space * (s + 1)) // ns)
