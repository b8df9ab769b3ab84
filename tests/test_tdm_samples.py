"""The sampled comparisons of tests/test_gpu_tdm.py, checked without a GPU: for the seeds that test uses at its three largest sizes the
checker alone must give between 3000 and 30000 sampled entries with terms, the condition the GPU test asserts again.  The lists come
from that test's own builders (host-side code only: ChemHost reads the integral file and names the HF determinant)."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import rdm2_checker as R2         # noqa: E402
from tests import tdm_checker as TC          # noqa: E402
from tests import test_gpu_tdm as T          # noqa: E402


@pytest.fixture(scope="module")
def chem_host():
    from sqmc_amd import host as H
    return H.ChemHost(T.FCIDUMP, 8, 4, "d2h")


@pytest.mark.parametrize("kind", ["sd", "neighbours"])
@pytest.mark.parametrize("n", T.SAMPLED)
def test_the_seeded_samples_are_large_enough(chem_host, n, kind):
    h = chem_host
    rng = random.Random(3000 + n + (0 if kind == "sd" else 50000))             # test_entries_chem's seed
    dets = T._sd_list(h, rng, n) if kind == "sd" else T._neighbours(rng, (int(h.hf_up), int(h.hf_dn)), h.norb, n)
    bra, ket = T._pair(rng, n)
    exp = TC.two_tdm(dets, bra, ket, h.norb, {b: T._Every8th(n) for b in R2.BLOCKS})
    sizes = {b: len(exp.terms[b]) for b in R2.BLOCKS}
    print("%s n = %d: %r sampled entries with terms" % (kind, n, sizes))
    assert 3000 <= sum(sizes.values()) <= 30000, sizes
    assert all(set(exp.terms[b]) <= exp.reached[b] for b in R2.BLOCKS)
    assert sum(len(v) for b in R2.BLOCKS for v in exp.terms[b].values()) > sum(sizes.values())      # entries with more than one term exist
