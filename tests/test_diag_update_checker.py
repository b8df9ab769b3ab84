"""tests/diag_update_checker.py on the CPU: the statement-by-statement update agrees with the brute-force H_aa within the derived
bound on every double excitation of a few sources (chemistry and electron gas, degenerate spin sectors included), and every
doctored update is rejected by that bound -- the comparison has the power tests/test_gpu_diag_update.py relies on."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import diag_update_checker as DU       # noqa: E402
from tests import proposal_checker as PC          # noqa: E402
from tests import test_proposal_unbiased as TU    # noqa: E402

DOCTORS = ("exchange_branch", "keep_r", "swap_pr")


def _case(request, which):
    sysm = request.getfixturevalue(which)
    chem = which.startswith("c2")
    H = TU.chem_checker(sysm) if chem else TU.heg_checker(sysm)
    return sysm, H, DU.ints_of(H, None if chem else sysm)


def _records(H, sources, stride=1):
    return [(s, pqrs, new) for s in sources for pqrs, new in DU.double_records(H, s)[::stride]]


@pytest.mark.parametrize("which,n_src,stride", [("c2_walk", 3, 3), ("heg14", 8, 1), ("heg57", 3, 1)])
def test_update_matches_brute_force_and_doctored_updates_do_not(request, which, n_src, stride):
    """C2: every 3rd double of HF and two seeded sources (the GPU test takes all of them); HEG: every momentum-conserving double"""
    sysm, H, ints = _case(request, which)
    nelec = sysm.nup + sysm.ndn
    src = DU.seeded_sources((sysm.hf_up, sysm.hf_dn), H.norb, sysm.nup, sysm.ndn, n_src)
    rec = _records(H, src, stride)
    kinds = {(r[1][0] <= H.norb, r[1][1] <= H.norb) for r in rec}
    assert kinds == {(True, True), (False, False), (True, False)}, kinds           # up-up, dn-dn, up-dn
    for s, pqrs, new in rec[:50]:
        assert DU.apply(s, pqrs, H.norb) == new
    want = DU.brute_many(H, [r[2] for r in rec])
    for k in range(0, len(rec), max(1, len(rec) // 40)):            # the vectorised brute force is hci_checker's second-quantised element
        h, n, sab = DU.brute(H, rec[k][2])
        assert abs(float(want[k]) - h) <= 2.0 * DU.U * abs(h), (rec[k], float(want[k]), h)
    fails, worst = DU.check(H, ints, rec, None, nelec, want=want)
    print("%s: %d records, clean update worst |delta| / bound = %.3g" % (which, len(rec), worst))
    assert not fails, fails[:3]
    k_max = max(DU.update(ints, H.norb, 0.0, pqrs, new[0], new[1])[2] for _, pqrs, new in rec)
    assert k_max <= 8 * nelec - 8 < DU.n_additions(nelec)
    for doctor in DOCTORS:
        fails, worst = DU.check(H, ints, rec, None, nelec, doctor, want=want)
        print("%s: doctored %-16s %6d of %d records outside the bound, worst |delta| / bound = %.3g" % (which, doctor, len(fails), len(rec), worst))
        assert fails and worst > 1e3, doctor


@pytest.mark.parametrize("nup,ndn", [(1, 1), (4, 0), (1, 3)])
def test_degenerate_spin_sectors(request, nup, ndn):
    """nup = 1 with ndn = 1: both loops skip everything; ndn = 0: one spin has no electrons at all; nup = 1, ndn = 3: no up-up pair"""
    sysm, H, ints = _case(request, "c2_walk")
    hf = ((1 << nup) - 1, (1 << ndn) - 1)
    rec = _records(H, DU.seeded_sources(hf, H.norb, nup, ndn, 2), 3)
    assert rec
    fails, worst = DU.check(H, ints, rec, None, nup + ndn)
    print("nup %d ndn %d: %d records, worst |delta| / bound = %.3g" % (nup, ndn, len(rec), worst))
    assert not fails, fails[:3]
    if nup == 1 and ndn == 1:
        assert all(DU.update(ints, H.norb, 0.0, pqrs, new[0], new[1])[2] == 6 for _, pqrs, new in rec)      # 4 + 2, no exchange, empty loops


def test_caches_belong_to_the_hamiltonian_not_to_its_id(heg14):
    """Hamiltonians built one after the other, each dropped before the next: an address is handed out again once its object is
    collected, and a cache keyed by id(H) then serves the new Hamiltonian the old one's tables.  Every one gets its own values;
    and an entry planted under a live Hamiltonian's id for another object is not believed."""
    from tests import hci_checker as HC
    dets = DU.seeded_sources((heg14.hf_up, heg14.hf_dn), heg14.norb, heg14.nup, heg14.ndn, 3)
    seen = set()
    for k in range(6):
        H = PC.HegH(heg14.k_vectors() / (1.0 + 0.25 * k), heg14.length_cell * (1.0 + 0.25 * k))          # the same gas in a larger cell
        own = [HC.diagonal(H, d)[0] for d in dets]
        seen.add(own[0])
        assert [DU.brute(H, d)[0] for d in dets] == own, k
        many = DU.brute_many(H, dets)
        assert all(abs(float(a) - b) <= 2.0 * DU.U * abs(b) for a, b in zip(many, own)), k
        del H
    assert len(seen) == 6          # the six cells really have different elements
    H = PC.HegH(heg14.k_vectors(), heg14.length_cell)
    DU._CACHES[id(H)] = (object(), {d: (1e9, 0, 0.0) for d in dets}, {})
    assert DU.brute(H, dets[0])[0] == HC.diagonal(H, dets[0])[0]


def test_bound_is_the_formula():
    assert DU.n_additions(8) == 72 and DU.n_additions(14) == 120
    assert DU.gamma(72) == 72 * DU.U / (1 - 72 * DU.U)
    assert DU.bound(-75.0, 25.0, 8) == DU.gamma(72) * 100.0
