"""CPU checks of proposal_method CauchySchwarz with time-reversal symmetry: the checker's time-symmetric move (tests/cauchy_ts_checker.py)
is unbiased against the oracle's time-symmetric Hamiltonian, the literal Cauchy-Schwarz arm of is_connected_chem departs from the move's
path mass exactly where tests/golden/README_cauchyschwarz_time_sym.md says, and a time-symmetric CauchySchwarz walk deck parses."""
import os
import re

import numpy as np
import pytest

from sqmc_amd.walk_run import parse_walk_deck
from tests import cauchy_checker as CC
from tests import cauchy_ts_checker as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FCIDUMP = os.path.join(GOLD, "C2_r1.24253_FCIDUMP")
TAU = 0.005314

# (z, hf_symmetry, n_core_orb): the c2_hci conventions, the 3pi_u deck's z = -1, and a frozen core
SYSTEMS = {"z+1": (1, 1, 0), "z-1": (-1, 2, 0), "z+1_core1": (1, 1, 1)}


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for name, (z, hs, nc) in SYSTEMS.items():
        s = oracle.ChemSystem(FCIDUMP, 8, 4, "d2h", time_sym=True, z=z, n_core_orb=nc, hf_mode=1, hf_symmetry=hs)
        cs = CC.CSTables(s.norb, s.nup, s.ndn, nc, list(s.orbsym()), s.prod(), s.integrals(), s.combine_2())
        out[name] = (s, cs, z)
    return out


def _level(iu, id_, ju, jd):
    return bin(iu ^ ju).count("1") // 2 + bin(id_ ^ jd).count("1") // 2


def _parents(s, cs, z):
    """representatives (up <= dn) that keep the core: HF, two singles, two doubles, an open-shell double and (z = +1) a double with up == dn"""
    hu, hd = s.hf_up, s.hf_dn
    cu, cd, _ = s.connected(hu, hd, with_elems=False)
    m = (1 << cs.nc) - 1
    pool = [(int(u), int(d)) for u, d in zip(cu, cd) if int(u) <= int(d) and (int(u), int(d)) != (hu, hd) and (int(u) & m) == m and (int(d) & m) == m]
    if z < 0:
        pool = [x for x in pool if x[0] != x[1]]
    singles = [x for x in pool if _level(hu, hd, *x) == 1 or _level(hd, hu, *x) == 1]
    doubles = [x for x in pool if x not in singles]
    rng = np.random.default_rng(5)
    out = [(hu, hd)]
    out += [singles[k] for k in rng.choice(len(singles), size=2, replace=False)]
    out += [doubles[k] for k in rng.choice(len(doubles), size=2, replace=False)]
    out.append(next(x for x in doubles if x[0] != x[1] and (x[0] & x[1]) != x[0] and x not in out))
    if z == 1:
        out.append(next(x for x in doubles if x[0] == x[1] and x != (hu, hd)))
    return out


def _ham(s):
    return lambda iu, id_, ju, jd, level: s.ham_chem(iu, id_, ju, jd, level)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_time_symmetric_move_is_unbiased(systems, name):
    """For every representative r != det_i: the sum over the move's paths ending at r or flip(r) of mass x weight_j equals
    -tau H_ts(det_i, r), H_ts from the oracle's hamiltonian_chem_time_sym (independent of the checker), within 1e-12 relative."""
    s, cs, z = systems[name]
    ham = _ham(s)
    parents = _parents(s, cs, z)
    assert len(parents) == (7 if z == 1 else 6)
    assert any(u == d for u, d in parents) == (z == 1)
    for iu, id_ in parents:
        paths, null, reported = cs.enumerate(iu, id_)
        acc, scale = {}, {}
        for p in paths:
            ju, jd = p[5]
            ru, rd, w = TS.finish(cs, z, TAU, iu, id_, ju, jd, p[0], reported[(ju, jd)], ham)
            if (min(ju, jd), max(ju, jd)) == (min(iu, id_), max(iu, id_)):
                assert w == 0.0
                continue
            assert ru <= rd
            acc[(ru, rd)] = acc.get((ru, rd), 0.0) + p[6] * w
            scale[(ru, rd)] = scale.get((ru, rd), 0.0) + abs(p[6] * w)
        cu, cd, _ = s.connected(iu, id_, with_elems=False)
        reps = {(min(int(u), int(d)), max(int(u), int(d))) for u, d in zip(cu, cd)} - {(iu, id_)}
        assert set(acc) <= reps
        m = (1 << cs.nc) - 1
        for r in reps:
            want = -TAU * s.ham(iu, id_, r[0], r[1])
            got = acc.get(r, 0.0)
            if (r[0] & m) != m or (r[1] & m) != m:          # outside the active space: never proposed
                assert got == 0.0
                continue
            tol = 1e-12 * max(abs(want), scale.get(r, 0.0)) + 1e-300
            assert abs(got - want) <= max(tol, 1e-12 * TAU * 1e-6), (name, iu, id_, r, got, want)


def _uu_mixed(cs, iu, id_, tu, td):
    """the branch README_cauchyschwarz_time_sym.md item 1 names: det_i -> target an up-up double whose holes differ in symmetry, with
    an occupied up orbital of the lower hole's symmetry (the loop at 2286-2289 runs)"""
    if id_ != td or bin(iu ^ tu).count("1") != 4:
        return False
    k, l = sorted(TS._bits(tu & ~iu))
    return cs.orbsym[k] != cs.orbsym[l] and any(cs.orbsym[x] == cs.orbsym[k] for x in TS._bits(iu))


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_literal_arm_departs_exactly_where_the_readme_says(systems, name):
    """Every (parent, det_j) with det_j a proposal of the move and flip(det_j) connected to det_i: the product's arm (det_i's tables,
    `+` at 2288) gives the move's own path mass of flip(det_j) within 1e-12; the literal arm (2288 as written) departs from it in
    exactly the up-up doubles with holes of different symmetry (item 1), and nowhere else."""
    s, cs, z = systems[name]
    ps, pd = cs.n_single / float(cs.n_total), cs.n_double / float(cs.n_total)
    n_dep = n_checked = 0
    for iu, id_ in _parents(s, cs, z):
        paths, _, _ = cs.enumerate(iu, id_)
        mass = TS.flip_mass(paths)
        for ju, jd in mass:
            if (jd, ju) == (iu, id_) or (ju, jd) == (iu, id_):
                continue
            conn, lev, p = TS.arm(cs, iu, id_, jd, ju)
            if not conn:
                assert mass.get((jd, ju), 0.0) == 0.0
                continue
            want = mass.get((jd, ju), 0.0)
            got = p * (ps if lev == 1 else pd)
            assert abs(got - want) <= 1e-12 * want, (name, iu, id_, ju, jd, got, want)
            lconn, llev, lp = TS.literal_arm(cs, iu, id_, jd, ju)
            assert (lconn, llev) == (conn, lev)
            lit = lp * (ps if lev == 1 else pd)
            departs = abs(lit - want) > 1e-12 * want
            assert departs == _uu_mixed(cs, iu, id_, jd, ju), (name, iu, id_, ju, jd, lit, want)
            n_dep += departs
            n_checked += 1
    assert n_checked > 300 and n_dep > 0


def test_stale_tables_depart_after_a_single(systems):
    """item 2: the arm reads cs_sqrt_prime* from module state that only the double branch of the move fills.  After a single from
    det_i whose flip is a double from det_i, the tables are another parent's: the literal arm then departs from the path mass; with
    det_i's own tables (what the product computes) it does not."""
    s, cs, z = systems["z+1"]
    ps, pd = cs.n_single / float(cs.n_total), cs.n_double / float(cs.n_total)
    parents = _parents(s, cs, z)
    other = TS.MoveTables(cs, *parents[0])
    n = 0
    for iu, id_ in parents[1:]:
        paths, _, _ = cs.enumerate(iu, id_)
        mass = TS.flip_mass(paths)
        for p in paths:
            if p[0] != 1:
                continue
            ju, jd = p[5]
            conn, lev, pown = TS.arm(cs, iu, id_, jd, ju)
            if not conn or lev != 2 or _uu_mixed(cs, iu, id_, jd, ju):
                continue
            want = mass[(jd, ju)]
            assert abs(pown * pd - want) <= 1e-12 * want
            _, _, pstale = TS.literal_arm(cs, iu, id_, jd, ju, tab=other)
            assert abs(pstale * pd - want) > 1e-9 * want, (iu, id_, ju, jd)
            n += 1
    assert n > 0


def test_move_stream_and_representatives(systems):
    """the checker's time-symmetric move lands on representatives and leaves the base move's stream untouched (the arm draws nothing)"""
    s, cs, z = systems["z+1"]
    ham = _ham(s)
    for iu, id_ in _parents(s, cs, z)[:4]:
        for k in range(200):
            st = CC.seed_state([k + 1, 33 * k % 4096, 77, 2 * k + 1])
            r1, r2 = CC.Rannyu(st), CC.Rannyu(st)
            lev, ju, jd, w = TS.move(cs, z, TAU, iu, id_, r1, ham)
            lev0, ju0, jd0, _ = cs.move(iu, id_, r2)
            assert r1.x == r2.x and lev == lev0
            if lev and w != 0.0:
                assert ju <= jd and (ju, jd) == (min(ju0, jd0), max(ju0, jd0))


# ------------------------------------------------------------------------------------------------ deck grammar
def _ts_deck(z=1):
    txt = open(os.path.join(GOLD, "C2_r1.24253_i_walk")).read()
    txt = re.sub(r"^uniform2(\s)", r"CauchySchwarz\1", txt, count=1, flags=re.M)
    return re.sub(r"^\.false\.(\s+time_sym)", ".true.\\1\n%d                                 z" % z, txt, count=1, flags=re.M)


@pytest.mark.parametrize("z", [1, -1])
def test_deck_accepts_cauchyschwarz_with_time_sym(z):
    d = parse_walk_deck(_ts_deck(z))
    assert d["proposal_method"] == "cauchyschwarz" and d["time_sym"] and d["z"] == z


def test_deck_still_refuses_cauchyschwarz_time_sym_with_hf_to_psit():
    with pytest.raises(SystemExit, match="hf_to_psit"):
        parse_walk_deck(_ts_deck().replace("f f 0.5 ", "t f 0.5 ", 1))
