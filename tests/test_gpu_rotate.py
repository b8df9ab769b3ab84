"""sqmc_gpu_rotate_integrals on the MI355X against the independent model of tests/rotate_checker.py: every packed entry within the derived
rounding bound at the edge sizes, exact cases compared with ==, the C2 fixture's symmetry zeros and invariants, full-CI invariance through
a second context, the refusals, and the deck runner's --rotate-integrals path."""
import ctypes as C
import io
import itertools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC     # noqa: E402
from tests import rotate_checker as RC       # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
BAD_ARG, UNSUPPORTED = -1, -3
EDGE_SIZES = [1, 2, 3, 15, 16, 17, 63, 64]


@pytest.fixture(scope="module")
def dev():
    import sqmc_amd
    sqmc_amd.set_device(0)
    return sqmc_amd


# ------------------------------------------------------------------------------------------------------------------ synthetic systems
def _write_fcidump(path, norb, nelec, keys, vals, hmat, core, orbsym=None):
    """keys: arrays P, Q, R, S (0-based, any order inside a class) of the two-body records; hmat[p][q] written for p >= q where non-zero"""
    P, Q, R, S = keys
    with open(path, "w") as f:
        f.write(" &FCI NORB=%d,NELEC=%d,MS2=0,\n  ORBSYM=%s,\n  ISYM=1,\n &END\n" % (norb, nelec, ",".join(str(s) for s in (orbsym or [1] * norb))))
        f.write("".join("%.17e %d %d %d %d\n" % t for t in zip(np.asarray(vals, float).tolist(), (P + 1).tolist(), (Q + 1).tolist(), (R + 1).tolist(), (S + 1).tolist())))
        for p in range(norb):
            for q in range(p + 1):
                if hmat[p][q] != 0.0:
                    f.write("%.17e %d %d 0 0\n" % (hmat[p][q], p + 1, q + 1))
        f.write("%.17e 0 0 0 0\n" % core)


def _context_order(h, norb, keys, vals, hmat, core):
    """the same integrals as RC.Integrals over the CONTEXT's orbitals: bit k of a determinant is the file's orbital orb_order[k + 1] (data)"""
    inv = np.asarray(h.orb_order_inv[1:norb + 1], np.int64) - 1          # file orbital (0-based) -> context orbital
    P, Q, R, S = (inv[x] for x in keys)
    a, b, c, d = np.maximum(P, Q), np.minimum(P, Q), np.maximum(R, S), np.minimum(R, S)
    swap = a * (a + 1) // 2 + b < c * (c + 1) // 2 + d
    a, b, c, d = np.where(swap, c, a), np.where(swap, d, b), np.where(swap, a, c), np.where(swap, b, d)
    two = dict(zip(zip(a.tolist(), b.tolist(), c.tolist(), d.tolist()), np.asarray(vals, float).tolist()))
    assert len(two) == len(vals)
    one = {}
    for p in range(norb):
        for q in range(p + 1):
            if hmat[p][q] != 0.0:
                i, j = int(inv[p]), int(inv[q])
                one[(max(i, j), min(i, j))] = float(hmat[p][q])
    return RC.Integrals(norb, one, two, float(core))


class _System:
    def __init__(self, h, ints, contexts):
        self.h, self.ints, self.norb, self._ctx = h, ints, h.norb, contexts
        self.g = h.gpu()
        contexts.append(self.g)
        self.two, self.one, self.core = RC.addresses(self.norb, h.combine_2)
        tri = np.tril_indices(self.norb)
        self.addressed = np.concatenate([self.two, self.one[tri], [self.core]])

    def fresh(self):
        g = self.h.gpu()
        self._ctx.append(g)
        return g


_SYS, _CTX = {}, []


def _dense(dev, tmp_path_factory, norb, nelec=2, nup=1):
    """dense random integrals on the canonical index set, c1; kept for the module (63 and 64 orbitals: 2 million records each)"""
    from sqmc_amd import host as H
    key = ("dense", norb, nelec)
    if key not in _SYS:
        rng = np.random.default_rng(1000 + norb)
        keys = RC.canonical_keys(norb)
        vals = rng.uniform(-1.0, 1.0, len(keys[0]))
        vals = np.where(np.abs(vals) < 1e-6, 1e-6, vals)                 # the readers leave out |value| <= 1e-9
        hmat = rng.uniform(-1.0, 1.0, (norb, norb))
        hmat = np.where(np.abs(hmat) < 1e-6, 1e-6, hmat)
        path = str(tmp_path_factory.mktemp("rot%d_%d" % (norb, nelec)) / "FCIDUMP")
        _write_fcidump(path, norb, nelec, keys, vals, hmat, -7.0625 - norb)
        h = H.ChemHost(path, nelec, nup, "c1")
        _SYS[key] = _System(h, _context_order(h, norb, keys, vals, hmat, -7.0625 - norb), _CTX)
        _SYS[key].path = path
    return _SYS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for g in _CTX:
        g.close()
    _CTX.clear(); _SYS.clear()


def _orthogonal(norb, seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((norb, norb)))[0]


def _check(s, U, exp, tag):
    got = s.g.rotate_integrals(U)
    assert got.shape == s.h.integrals.shape and got.dtype == np.float64
    fails, worst = RC.compare(exp, got, s.h.combine_2)
    print("%s norb = %d: worst |delta| / bound = %.4f" % (tag, s.norb, worst))
    assert not fails, fails[:4]
    assert not got[RC.unaddressed(s.norb, s.h.combine_2, len(got))].any()          # index 0, the pair indices nothing addresses
    assert got[s.core] == s.h.integrals[s.core] == exp.core
    return got


# ----------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("norb", EDGE_SIZES)
def test_edge_sizes(dev, tmp_path_factory, norb):
    """dense integrals, dense orthogonal U: one pair; pair-index arithmetic; a 16-wide tile's seam; the ABI limit with the norb + 1 = 65
    one-body slot and 96 KB of LDS"""
    s = _dense(dev, tmp_path_factory, norb)
    U = _orthogonal(norb, 2000 + norb)
    exp = RC.transform_exact(s.ints, U) if norb <= 3 else RC.transform_fast(s.ints, U)
    got = _check(s, U, exp, "dense")
    assert np.count_nonzero(got[s.addressed]) == len(s.addressed)
    # the context's own integrals are as they were: the identity still returns them
    assert np.array_equal(s.g.rotate_integrals(np.eye(norb))[s.addressed], s.h.integrals[s.addressed])


@pytest.mark.parametrize("norb", [17, 64])
def test_identity_returns_the_input_bits(dev, tmp_path_factory, norb):
    s = _dense(dev, tmp_path_factory, norb)
    got = s.g.rotate_integrals(np.eye(norb))
    assert np.array_equal(got[s.addressed], s.h.integrals[s.addressed])
    assert not got[RC.unaddressed(norb, s.h.combine_2, len(got))].any()


@pytest.mark.parametrize("norb", [17, 64])
@pytest.mark.parametrize("kind", ["seeded", "reversal"])
def test_signed_permutation_relabels_exactly(dev, tmp_path_factory, norb, kind):
    s = _dense(dev, tmp_path_factory, norb)
    if kind == "seeded":
        rng = np.random.default_rng(3000 + norb)
        perm, sign = rng.permutation(norb), rng.choice([-1.0, 1.0], norb)
    else:
        perm, sign = np.arange(norb)[::-1].copy(), np.where(np.arange(norb) % 2, -1.0, 1.0)
    U = np.zeros((norb, norb))
    U[perm, np.arange(norb)] = sign                         # new orbital p = sign[p] * old orbital perm[p]
    got = s.g.rotate_integrals(U)
    c2, src = s.h.combine_2, s.h.integrals
    P, Q, R, S = RC.canonical_keys(norb)
    want = (sign[P] * sign[Q] * sign[R] * sign[S]) * src[RC.packed_index(c2, perm[P] + 1, perm[Q] + 1, perm[R] + 1, perm[S] + 1)]
    assert (got[s.two] == want).all()
    p, q = np.tril_indices(norb)
    n1 = np.full_like(p, norb + 1)
    assert (got[s.one[p, q]] == sign[p] * sign[q] * src[RC.packed_index(c2, perm[p] + 1, perm[q] + 1, n1, n1)]).all()
    assert got[s.core] == src[s.core] and (sign < 0).any() and (perm != np.arange(norb)).any()


GIVENS = [(0, 63), (15, 16), (31, 32), (47, 48)]


def test_givens_rotations_across_tile_seams(dev, tmp_path_factory):
    """norb = 64, 2 x 2 rotations on four orbital pairs that straddle the register tiles and the first / last orbital, a few hundred
    integrals that touch them: the exact sparse model, and bit-equal entries where no index is a rotated orbital"""
    from sqmc_amd import host as H
    norb = 64
    rng = np.random.default_rng(4000)
    hot = sorted(set(itertools.chain(*GIVENS)))
    keys = set()
    while len(keys) < 300:
        idx = [int(x) for x in rng.integers(0, norb, 4)]
        if len(keys) < 260:
            idx[int(rng.integers(0, 4))] = int(rng.choice(hot))
        keys.add(RC.canon(*idx))
    keys = sorted(keys)
    ka = tuple(np.array([k[i] for k in keys], np.int64) for i in range(4))
    vals = rng.uniform(-0.05, 0.05, len(keys))
    vals = np.where(np.abs(vals) < 1e-6, 1e-6, vals)
    hmat = np.diag(10.0 * (1 + np.arange(norb)))             # orbital energies far apart: the context keeps the file's order
    for p, q in [(63, 0), (16, 15), (32, 31), (48, 47), (40, 3), (63, 62)]:
        hmat[p][q] = rng.uniform(-1, 1)
    path = str(tmp_path_factory.mktemp("givens") / "FCIDUMP")
    _write_fcidump(path, norb, 2, ka, vals, hmat, 0.5)
    h = H.ChemHost(path, 2, 1, "c1")
    assert list(h.orb_order[1:norb + 1]) == list(range(1, norb + 1))
    s = _System(h, _context_order(h, norb, ka, vals, hmat, 0.5), _CTX)
    U = np.eye(norb)
    for k, (i, j) in enumerate(GIVENS):
        c, sn = math.cos(0.3 + 0.4 * k), math.sin(0.3 + 0.4 * k)
        U[i, i], U[j, j], U[i, j], U[j, i] = c, c, -sn, sn
    got = _check(s, U, RC.transform_sparse(s.ints, U), "givens")
    P, Q, R, S = RC.canonical_keys(norb)
    cold = ~(np.isin(P, hot) | np.isin(Q, hot) | np.isin(R, hot) | np.isin(S, hot))
    assert np.array_equal(got[s.two[cold]], h.integrals[s.two[cold]]) and np.count_nonzero(h.integrals[s.two[cold]]) >= 20
    p, q = np.tril_indices(norb)
    cold1 = ~(np.isin(p, hot) | np.isin(q, hot))
    assert np.array_equal(got[s.one[p, q][cold1]], h.integrals[s.one[p, q][cold1]])
    assert got[s.one[40, 3]] == h.integrals[s.one[40, 3]] != 0.0 and got[s.one[63, 62]] != h.integrals[s.one[63, 62]] != 0.0


def test_non_orthogonal_matrix_is_a_congruence(dev, tmp_path_factory):
    s = _dense(dev, tmp_path_factory, 5, nelec=4, nup=2)
    U = np.random.default_rng(5000).uniform(-1.0, 1.0, (5, 5))
    assert abs(np.linalg.det(U)) > 1e-3 and np.abs(U.T @ U - np.eye(5)).max() > 0.1
    _check(s, U, RC.transform_exact(s.ints, U), "non-orthogonal")


@pytest.mark.parametrize("norb", [26, 64])
def test_same_bits_call_to_call_and_context_to_context(dev, tmp_path_factory, norb):
    s = _dense(dev, tmp_path_factory, norb)
    U = _orthogonal(norb, 6000 + norb)
    a, b = s.g.rotate_integrals(U), s.g.rotate_integrals(U)
    c = s.fresh().rotate_integrals(U)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.count_nonzero(a[s.addressed]) == len(s.addressed)


# ------------------------------------------------------------------------------------------------------------------------- C2, the deck
def _deck_text(natorb):
    t = open(DECK).read().replace("1e-3  1e-7", "5e-3  1e-5").replace("eps_var_sched=2*2e-3", "eps_var_sched=2*1e-2")
    assert "5e-3  1e-5" in t and "2*1e-2" in t
    return t + ("&natorb get_natorbs=.true. /\n" if natorb else "")


@pytest.fixture(scope="module")
def c2_run(dev, tmp_path_factory):
    """the small C2 deck with &natorb, run once with the rotation switched on"""
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    path = str(tmp_path_factory.mktemp("c2deck") / "F")
    buf = io.StringIO()
    res = R.run_hci(R.parse_hci_deck(_deck_text(True)), FCIDUMP, out=buf, natorb_fcidump=path)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    return res, buf.getvalue().splitlines(), path, h


def _c2_integrals(h):
    norb, one, two, core = PC.read_fcidump(FCIDUMP)
    inv = {int(h.orb_order[i]): i - 1 for i in range(1, norb + 1)}
    return RC.Integrals(norb, {(max(inv[p], inv[q]), min(inv[p], inv[q])): v for (p, q), v in one.items()},
                        {RC.canon(inv[p], inv[q], inv[r], inv[s]): v for (p, q, r, s), v in two.items()}, core)


def test_c2_natural_orbitals(dev, c2_run):
    res, _, _, h = c2_run
    norb, U, got, c2 = 26, res["vectors"], res["natorb_integrals"], h.combine_2
    assert U.shape == (norb, norb) and np.abs(U.T @ U - np.eye(norb)).max() < 1e-12
    ints = _c2_integrals(h)
    exp = RC.transform_fast(ints, U)
    fails, worst = RC.compare(exp, got, c2)
    print("C2 natural orbitals: worst |delta| / bound = %.4f" % worst)
    assert not fails, fails[:4]
    assert not got[RC.unaddressed(norb, c2, len(got))].any()
    # symmetry: d2h irreps multiply by xor of (label - 1); a forbidden entry is a sum of products with an exact zero
    sym = np.asarray(h.orbsym[1:norb + 1], np.int64) - 1
    a2, a1, ac = RC.addresses(norb, c2)
    P, Q, R, S = RC.canonical_keys(norb)
    forbidden = (sym[P] ^ sym[Q] ^ sym[R] ^ sym[S]) != 0
    assert forbidden.sum() > 1000 and not got[a2[forbidden]].any() and np.count_nonzero(got[a2[~forbidden]]) > 1000
    p, q = np.tril_indices(norb)
    assert not got[a1[p, q][sym[p] != sym[q]]].any()
    # invariants of an orthogonal rotation, each within the summed bounds of the entries that enter it
    rg = range(norb)
    scale = exp.factor * (norb + 1) * RC.U53 * exp._inflate()
    at = lambda i, j, k, l: got[int(RC.packed_index(c2, *(np.array(x + 1) for x in (i, j, k, l))))]
    tr_new, tr_old = math.fsum(got[a1[i, i]] for i in rg), math.fsum(ints.h(i, i) for i in rg)
    b_tr = 2.0 * scale * math.fsum(float(exp.one_S[i, i]) for i in rg)
    j_new, j_old = math.fsum(at(i, i, j, j) for i in rg for j in rg), math.fsum(ints.v(i, i, j, j) for i in rg for j in rg)
    b_j = 4.0 * scale * math.fsum(float(exp.two_S[RC.key_position(RC.canon(i, i, j, j))]) for i in rg for j in rg)
    k_new, k_old = math.fsum(at(i, j, j, i) for i in rg for j in rg), math.fsum(ints.v(i, j, j, i) for i in rg for j in rg)
    b_k = 4.0 * scale * math.fsum(float(exp.two_S[RC.key_position(RC.canon(i, j, j, i))]) for i in rg for j in rg)
    print("tr h: %.3e of %.3e;  sum (PP|QQ): %.3e of %.3e;  sum (PQ|QP): %.3e of %.3e" % (abs(tr_new - tr_old), b_tr, abs(j_new - j_old), b_j, abs(k_new - k_old), b_k))
    assert abs(tr_new - tr_old) <= b_tr and abs(j_new - j_old) <= b_j and abs(k_new - k_old) <= b_k


def test_deck_rotates_and_writes_the_file(dev, c2_run, tmp_path):
    from sqmc_amd import host as H
    from sqmc_amd import run as R
    res, lines, path, h = c2_run
    marks = ["Eigenvalues of 1RDM:", "Rotating integrals to new natural orbitals", "Done computing new integrals. Dumping new integrals into file " + path]
    at = [lines.index(m) for m in marks]
    assert at == sorted(at) and lines[-1] == marks[-1] and lines[at[1] - 1] == ""
    assert R.NATORB_STOP not in lines and not any("not built" in l for l in lines)
    assert not any("PT energy lowering" in l or "Total energy" in l for l in lines)
    assert res["natorb_fcidump"] == path
    g = h.gpu()
    try:
        assert np.array_equal(g.rotate_integrals(res["vectors"]), res["natorb_integrals"])
    finally:
        g.close()
    # the file
    head = open(path).read().split("\n", 4)[:4]
    assert head[0] == "&FCI NORB=   26, NELEC=    8, MS2=0" and head[2:] == ["ISYM=1", "&END"]
    norb, orbsym, _, _ = H.read_fcidump(path)
    assert norb == 26 and orbsym == H.read_fcidump(FCIDUMP)[1] and head[1] == "ORBSYM=" + "".join("%3d" % x for x in orbsym)
    h2 = H.ChemHost(path, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    # h2's integrals back at the packed result's addresses: context orbital of h -> file label -> context orbital of h2
    packed = res["natorb_integrals"]
    to2 = np.zeros(norb + 2, np.int64)
    to2[1:norb + 1] = h2.orb_order_inv[h.orb_order[1:norb + 1]]
    to2[norb + 1] = norb + 1
    a2, a1, ac = RC.addresses(norb, h.combine_2)
    kp, kq, kr, ks = (x + 1 for x in RC.canonical_keys(norb))
    p, q = (x + 1 for x in np.tril_indices(norb))
    n1 = np.full_like(p, norb + 1)
    mine = np.concatenate([packed[a2], packed[a1[p - 1, q - 1]], [packed[ac]]])
    theirs = np.concatenate([h2.integrals[RC.packed_index(h2.combine_2, to2[kp], to2[kq], to2[kr], to2[ks])],
                             h2.integrals[RC.packed_index(h2.combine_2, to2[p], to2[q], n1, n1)], [h2.integrals[-1]]])
    big = np.abs(mine) > 1e-8
    assert big.sum() > 1000 and (np.abs(theirs[big] - mine[big]) <= 5e-13 * np.abs(mine[big])).all()
    assert not theirs[~big].any()
    # a second run onto the same path is refused
    with pytest.raises(FileExistsError):
        R.run_hci(R.parse_hci_deck(_deck_text(True)), FCIDUMP, out=io.StringIO(), natorb_fcidump=path)
    # without the switch nothing changes: the run ends on NATORB_STOP
    buf = io.StringIO()
    res0 = R.run_hci(R.parse_hci_deck(_deck_text(True)), FCIDUMP, out=buf)
    l0 = buf.getvalue().splitlines()
    assert l0[-1] == R.NATORB_STOP and "natorb_integrals" not in res0 and not any(l.startswith("Rotating integrals") for l in l0)
    assert l0[:len(l0) - 2] == lines[:at[1] - 1]


# --------------------------------------------------------------------------------------------------------------- full-CI invariance
class _TableH(PC.Hamiltonian):
    """t / v from functions of the context's orbitals, diagonal in spin"""

    def __init__(self, norb, one, two, const=0.0):
        self.norb, self._one, self._two, self.const = norb, one, two, const

    def t(self, P, Q):
        n = self.norb
        return self._one(P % n, Q % n) if P // n == Q // n else 0.0

    def v(self, P, Q, R, S):
        n = self.norb
        return self._two(P % n, Q % n, R % n, S % n) if P // n == Q // n and R // n == S // n else 0.0


def test_full_ci_spectrum_is_invariant(dev, tmp_path_factory, tmp_path):
    """4 electrons in 5 orbitals, 100 determinants: the spectra of H in the old and in the rotated integrals agree within the Frobenius
    norm of the element-wise bound (Weyl), and the rotated context's elements are those of the integrals it was given"""
    norb = 5
    s = _dense(dev, tmp_path_factory, norb, nelec=4, nup=2)
    U = _orthogonal(norb, 7000)
    rot = s.g.rotate_integrals(U)
    h2 = s.h.with_integrals(rot)
    g2 = h2.gpu()
    _CTX.append(g2)
    strings = [sum(1 << k for k in c) for c in itertools.combinations(range(norb), 2)]
    dets = [(u, d) for u in strings for d in strings]
    assert len(dets) == 100
    iu = np.array([a[0] for a in dets for _ in dets], np.uint64); id_ = np.array([a[1] for a in dets for _ in dets], np.uint64)
    ju = np.array([b[0] for _ in dets for b in dets], np.uint64); jd = np.array([b[1] for _ in dets for b in dets], np.uint64)
    H1 = s.g.hamiltonian_batch(iu, id_, ju, jd).reshape(100, 100)
    H2 = g2.hamiltonian_batch(iu, id_, ju, jd).reshape(100, 100)
    assert np.array_equal(H1, H1.T) or np.abs(H1 - H1.T).max() < 1e-13
    # the rotated array as a full-precision FCIDUMP of this test's own making, read by the checker's reader
    order = [int(s.h.orb_order[i]) for i in range(1, norb + 1)]
    lab = np.array(order, np.int64) - 1
    P, Q, R, S = RC.canonical_keys(norb)
    hm = np.zeros((norb, norb))
    for p in range(norb):
        for q in range(p + 1):
            a, b = max(lab[p], lab[q]), min(lab[p], lab[q])
            hm[a][b] = rot[s.one[p, q]]
    path = str(tmp_path / "ROTATED")
    _write_fcidump(path, norb, 4, (lab[P], lab[Q], lab[R], lab[S]), rot[s.two], hm, rot[s.core])
    Hc = PC.ChemH(path, order)
    exp = RC.transform_exact(s.ints, U)
    Hb = _TableH(norb, exp.one_bound, exp.bound)
    B = np.zeros((100, 100))
    worst = 0.0
    for i, (au, ad) in enumerate(dets):
        for j, (bu, bd) in enumerate(dets):
            if j < i:
                B[i, j] = B[j, i]
                continue
            val, nt, sa = Hc.element(au, ad, bu, bd)
            rb = PC.rounding_bound(max(nt, 1), sa)
            assert abs(H2[i, j] - val) <= rb and abs(H2[j, i] - val) <= rb, (i, j, H2[i, j], val, rb)
            worst = max(worst, abs(H2[i, j] - val) / rb) if rb > 0 else worst
            B[i, j] = Hb.element(au, ad, bu, bd)[2] + rb
    e1, e2 = np.linalg.eigvalsh((H1 + H1.T) / 2), np.linalg.eigvalsh((H2 + H2.T) / 2)
    nb = float(np.linalg.norm(B))
    print("full CI: max |E - E'| = %.3e, ||B||_F = %.3e; elements vs own FCIDUMP: worst |delta| / rounding bound = %.3f" % (np.abs(e1 - e2).max(), nb, worst))
    assert np.abs(e1 - e2).max() <= nb
    assert np.abs(H1 - H2).max() > 1e-3                     # a real rotation: the matrices differ, the spectra do not


# ----------------------------------------------------------------------------------------------------------------------- refusals
def _raw(g, rot, out):
    g.L.sqmc_gpu_rotate_integrals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return g.L.sqmc_gpu_rotate_integrals(g.h, None if rot is None else rot.ctypes.data_as(C.c_void_p), None if out is None else out.ctypes.data_as(C.c_void_p))


def test_refusals_leave_the_output_untouched(dev, tmp_path_factory):
    from sqmc_amd import host as H
    for make in (lambda: H.HegHost(3, 0.5, 14, 7, 1.49).gpu(), lambda: H.HubbardHost(4, 4, True, 8, 8).gpu(), lambda: H.HubbardKHost(4, 4, 8, 8).gpu()):
        g = make()
        try:
            out = np.full(4096, 777.25)
            assert _raw(g, np.eye(g.norb), out) == UNSUPPORTED and (out == 777.25).all()
            with pytest.raises(dev.SqmcGpuError) as e:
                g.rotate_integrals(np.eye(g.norb))
            assert e.value.code == UNSUPPORTED
        finally:
            g.close()
    s = _dense(dev, tmp_path_factory, 5, nelec=4, nup=2)
    out = np.full(len(s.h.integrals), 777.25)
    assert _raw(s.g, None, out) == BAD_ARG and _raw(s.g, np.eye(5), None) == BAD_ARG
    for bad in (np.nan, np.inf, -np.inf):
        U = np.eye(5)
        U[3, 1] = bad
        assert _raw(s.g, U, out) == BAD_ARG
        with pytest.raises(dev.SqmcGpuError) as e:
            s.g.rotate_integrals(U)
        assert e.value.code == BAD_ARG
    assert (out == 777.25).all()
    with pytest.raises(ValueError):
        s.g.rotate_integrals(np.eye(4))
    assert _raw(s.g, np.eye(5), out) == 0 and np.array_equal(out[s.addressed], s.h.integrals[s.addressed])          # and the context still works
