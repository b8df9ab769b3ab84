"""CPU checks of proposal_method CauchySchwarz: the checker's exact path enumerator against the move it restates
(path masses, reported proposal probabilities, reach), rannyu as 48-bit arithmetic, the deck grammar and the
reference's stop and clamp on negative exchange integrals."""
import json
import os
import re

import numpy as np
import pytest

from sqmc_amd import host as H
from sqmc_amd.walk_run import parse_walk_deck
from tests import cauchy_checker as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FCIDUMP = os.path.join(GOLD, "C2_r1.24253_FCIDUMP")

SYSTEMS = {"c2_8e": (8, 4, 0), "c2_10e": (10, 5, 0), "c2_8e_core1": (8, 4, 1)}


def _host(name):
    nelec, nup, nc = SYSTEMS[name]
    return H.ChemHost(FCIDUMP, nelec, nup, "d2h", n_core_orb=nc)


def _parents(h, n_extra=4, seed=7):
    """HF, then singles, doubles and open-shell determinants drawn from its connections"""
    up, dn = h.connected_all(h.hf_up, h.hf_dn)
    rng = np.random.default_rng(seed)
    exc = lambda u, d: bin(int(u) ^ h.hf_up).count("1") // 2 + bin(int(d) ^ h.hf_dn).count("1") // 2
    pool = [(int(u), int(d)) for u, d in zip(up, dn) if (int(u), int(d)) != (h.hf_up, h.hf_dn)]
    singles = [x for x in pool if exc(*x) == 1]
    doubles = [x for x in pool if exc(*x) == 2]
    out = [(h.hf_up, h.hf_dn)]
    for lst in (singles, doubles):
        for k in rng.choice(len(lst), size=n_extra // 2, replace=False):
            out.append(lst[k])
    opened = [x for x in doubles if x[0] != x[1] and bin(x[0]).count("1") == bin(x[1]).count("1")]
    out.append(opened[len(opened) // 3])
    return out


def _core_kept(h, u, d):
    m = (1 << h.n_core_orb) - 1
    return (u & m) == m and (d & m) == m


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_enumerator_masses_probabilities_and_reach(name):
    h = _host(name)
    cs = CC.from_host(h)
    assert cs.n_clamped == 0              # every exchange integral of the C2 file is >= 0.00235
    parents = _parents(h)
    assert len(parents) >= 5
    for iu, id_ in parents:
        paths, null, reported = cs.enumerate(iu, id_)
        total = sum(p[-1] for p in paths) + null
        assert abs(total - 1.0) < 1e-12, (name, iu, id_, total)
        mass = {}
        for p in paths:
            mass[p[5]] = mass.get(p[5], 0.0) + p[6]
        assert set(mass) == set(reported)
        for dj, m in mass.items():
            assert abs(m - reported[dj]) < 1e-12, (name, iu, id_, dj, m, reported[dj])
        # every symmetry-allowed single and double that keeps the core is reachable (a superset of those with |H_ij| > 0)
        cu, cd = h.connected_all(iu, id_)
        for u, d in zip(cu, cd):
            u, d = int(u), int(d)
            if (u, d) == (iu, id_) or not _core_kept(h, u, d):
                continue
            assert mass.get((u, d), 0.0) > 0.0, (name, iu, id_, u, d)
        assert set(mass) <= {(int(u), int(d)) for u, d in zip(cu, cd)}


def test_move_reports_the_enumerated_probability():
    """single draws of the move land on enumerated determinants with the enumerated proposal probability"""
    h = _host("c2_8e")
    cs = CC.from_host(h)
    for iu, id_ in _parents(h)[:3]:
        _, _, reported = cs.enumerate(iu, id_)
        for k in range(300):
            r = CC.Rannyu(CC.seed_state([k + 1, 17 * k % 4096, 3001, 2 * k + 1]))
            lev, ju, jd, p = cs.move(iu, id_, r)
            if lev == 0:
                continue
            assert p == pytest.approx(reported[(ju, jd)], rel=1e-12, abs=0)


def test_fall_through_is_a_null_move():
    """decision 2 on the checker: a search whose cumulative sum stays below its draw returns None, and the move is then a null move"""
    h = _host("c2_8e")
    cs = CC.from_host(h)
    assert cs._search([0.25, 0.25, 0.4999999999999], 1.0 - 2.0 ** -48) is None and cs.fell_through
    cs.fell_through = False
    assert cs._search([0.25, 0.25, 0.5], 1.0 - 2.0 ** -48) == 2 and not cs.fell_through


def test_no_search_falls_through_on_the_shipped_systems():
    """On C2 every cumulative search of the move ends within 1.1e-15 of 1 from above or below, closer than the largest draw's
    distance to 1 (2^-48 = 3.6e-15): a draw of (2^48-1)/2^48 is always found, so decision 2 never acts here.  States whose k-th
    draw is that largest value (k = 1..6, the LCG's modular inverse) give no null move by fall-through, from HF and from its
    connections."""
    inv = pow(CC.LCG_MULT, -1, 1 << 48)
    for name in ("c2_8e", "c2_8e_core1"):
        h = _host(name)
        cs = CC.from_host(h)
        cu, cd = h.connected_all(h.hf_up, h.hf_dn)
        states, x = [], CC.MASK48
        for _ in range(6):
            x = (x * inv) & CC.MASK48
            states.append(x)
        for u, d in [(h.hf_up, h.hf_dn)] + list(zip(cu.tolist(), cd.tolist()))[:300]:
            for st in states:
                cs.move(int(u), int(d), CC.Rannyu(st))
                assert not cs.fell_through, (name, u, d, st)
            ou, od, act, csp, s = cs._electrons(int(u), int(d))
            ep = 0.0
            for v in csp:
                ep = ep + v / s
            assert abs(ep - 1.0) < 1.2e-15


def test_rannyu_is_the_reference_stream():
    gold = json.load(open(os.path.join(GOLD, "rannyu.json")))
    for rec in gold:
        r = CC.Rannyu(CC.seed_state(rec["seed"]))
        assert [r.draw().hex() for _ in range(len(rec["hex"]))] == rec["hex"]


# ------------------------------------------------------------------------------------------------ deck grammar
def _deck(name, token):
    txt = open(os.path.join(GOLD, name)).read()
    return re.sub(r"^uniform2(\s)", token + r"\1", txt, count=1, flags=re.M)


def test_deck_accepts_cauchyschwarz_for_chem():
    d = parse_walk_deck(_deck("C2_r1.24253_i_walk", "CauchySchwarz"))
    assert d["proposal_method"] == "cauchyschwarz" and d["hamiltonian_type"] == "chem"


@pytest.mark.parametrize("name", ["heg14_i_walk", "hubbard4x4_i_walk"])
def test_deck_refuses_cauchyschwarz_outside_chem(name):
    with pytest.raises(SystemExit, match="not on the GPU path"):
        parse_walk_deck(_deck(name, "CauchySchwarz"))


def test_deck_refuses_cauchyschwarz_with_hf_to_psit():
    txt = _deck("C2_r1.24253_i_walk", "CauchySchwarz").replace("f f 0.5 ", "t f 0.5 ", 1)
    with pytest.raises(SystemExit, match="hf_to_psit"):
        parse_walk_deck(txt)


def test_deck_refuses_cauchyschwarz_with_importance_sampling():
    txt = _deck("C2_r1.24253_i_walk", "CauchySchwarz").replace("CauchySchwarz 0 1.", "CauchySchwarz 1 1.", 1)
    with pytest.raises(SystemExit, match="importance_sampling"):
        parse_walk_deck(txt)


def test_hosts_refuse_cauchyschwarz_outside_chem():
    for cls in (H.HegHost, H.HubbardHost):          # refused before any context is made
        with pytest.raises(ValueError, match="chemistry only"):
            cls.gpu(object.__new__(cls), proposal="cauchyschwarz")


def _fcidump_with_exchange(tmp_path, value):
    """the C2 file with its first exchange integral (ij|ij), i != j, replaced by `value`"""
    lines = open(FCIDUMP).read().splitlines(True)
    for k, l in enumerate(lines):
        t = l.split()
        if len(t) == 5 and not l.lstrip().startswith("&"):
            try:
                i, j, a, b = (int(x) for x in t[1:])
            except ValueError:
                continue
            if i == a and j == b and i != j and i > 0 and j > 0:
                lines[k] = " %.16e %d %d %d %d\n" % (value, i, j, a, b)
                out = tmp_path / "FCIDUMP"
                out.write_text("".join(lines))
                return str(out), (i, j)
    raise AssertionError("no exchange integral in the file")


def test_negative_exchange_integral_stops(tmp_path):
    path, _ = _fcidump_with_exchange(tmp_path, -1e-5)
    h = H.ChemHost(path, 8, 4, "d2h")
    with pytest.raises(ValueError, match="Negative integrals!"):
        h.cauchy_schwarz_clamp()
    with pytest.raises(CC.NegativeIntegrals):
        CC.from_host(h)


def test_slightly_negative_exchange_integral_is_clamped(tmp_path):
    path, (i, j) = _fcidump_with_exchange(tmp_path, -1e-8)
    h = H.ChemHost(path, 8, 4, "d2h")
    i, j = int(h.orb_order_inv[i]), int(h.orb_order_inv[j])      # file orbitals -> the sorted order (sort_integrals)
    cs = CC.from_host(h)                      # the checker on an unclamped copy
    assert cs.n_clamped == 1 and cs.sq[i][j] == 0.0 and cs.sq[j][i] == 0.0
    assert h.cauchy_schwarz_clamp() == 1
    a = int(h.combine_2[i, j])
    assert h.integrals[a * (a - 1) // 2 + a] == 0.0
    assert h.cauchy_schwarz_clamp() == 0      # idempotent
    d = parse_walk_deck(_deck("C2_r1.24253_i_walk", "CauchySchwarz"))
    assert d["proposal_method"] == "cauchyschwarz"


def test_stop_threshold_is_the_default_real_literal():
    assert CC.STOP_BELOW == -9.999999974752427e-07
