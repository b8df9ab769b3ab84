"""The bucket-boundary blocks of the short-list tail (bk_positions_block / bk_next_block, sqmc_amd/csrc/bucket_partition.h) through
the door sqmc_gpu_debug_bucket_boundaries, against the independent model of tests/boundaries_checker.py: positions from
np.searchsorted, the prefix by a float64 loop, the partition point by a linear scan.  Integers: agreement is exact."""
import numpy as np
import pytest

import boundaries_checker as BC

pytestmark = pytest.mark.gpu
CASES = BC.cases()


@pytest.fixture(scope="module")
def ctx():
    import sqmc_amd
    sqmc_amd.set_device(0)
    g = sqmc_amd.GpuChem.hubbard(3, 3, False, 2, 2, 1.0, 4.0)      # the door needs a context's stream, nothing of its model
    yield g
    g.close()


@pytest.fixture(scope="module")
def expected():
    """the model's answers, computed once"""
    out = {}
    for name, (c, _) in CASES.items():
        pos = BC.positions(c["keys"], c["B"], c["kb"]) if c["kb"] is not None else None
        out[name] = (pos,) + BC.next_boundaries(c["keys"], c["B"], c["kb_prev"], c["pos_prev"], c["scount"])[:2]
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_boundaries_match_model(ctx, expected, name):
    c = CASES[name][0]
    pos, kb_out, hint_out = ctx.debug_bucket_boundaries(c["keys"], c["B"], kb=c["kb"], hint=c["hint"], kb_prev=c["kb_prev"], pos_prev=c["pos_prev"],
                                                        scount=c["scount"])
    e_pos, e_kb, e_hint = expected[name]
    if e_pos is None:
        assert pos is None
    else:
        assert np.array_equal(pos, e_pos), np.flatnonzero(pos != e_pos)
    assert np.array_equal(hint_out, e_hint), np.flatnonzero(hint_out != e_hint)
    assert np.array_equal(kb_out, e_kb), np.flatnonzero(kb_out != e_kb)


def test_positions_alone(ctx, expected):
    """a launch that only looks for positions (no next boundaries asked for) writes the same positions"""
    c = CASES["hint+385"][0]
    pos, kb_out, hint_out = ctx.debug_bucket_boundaries(c["keys"], c["B"], kb=c["kb"], hint=c["hint"], want_next=False)
    assert kb_out is None and hint_out is None and np.array_equal(pos, expected["hint+385"][0])
