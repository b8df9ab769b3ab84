"""The model the GPU boundary tests compare against (tests/boundaries_checker.py), checked on its own: its outputs are ordered, its
fallback fires exactly when a rule is broken, its linear scans agree with plain bisections, and every case built for a rule meets it."""
import numpy as np
import pytest

import boundaries_checker as BC

CASES = BC.cases()


def _random_case(seed):
    rng = np.random.default_rng(seed)
    B = int(rng.choice([2, 3, 5, 17, 64]))
    n0 = int(rng.integers(max(2 * B, 40), 1500))
    c = BC.base_case(n0, B, seed, spread=int(rng.choice([1, 50, 3000])), dup=bool(seed % 3 == 0))
    c["scount"][rng.integers(0, B)] = 0
    return c


@pytest.mark.parametrize("seed", range(40))
def test_linear_scan_agrees_with_bisection(seed):
    c = _random_case(seed)
    a = BC.next_boundaries(c["keys"], c["B"], c["kb_prev"], c["pos_prev"], c["scount"], point=BC.partition_point_linear)
    b = BC.next_boundaries(c["keys"], c["B"], c["kb_prev"], c["pos_prev"], c["scount"], point=BC.partition_point_bisect)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    pos = BC.positions(c["keys"], c["B"], c["kb"])
    for j in range(1, c["B"]):                       # a lower bound by bisection
        lo, hi = 0, len(c["keys"])
        while lo < hi:
            m = (lo + hi) >> 1
            if c["keys"][m] < c["kb"][j]:
                lo = m + 1
            else:
                hi = m
        assert pos[j] == lo


@pytest.mark.parametrize("seed", range(40))
def test_output_is_ordered_and_fallback_is_equal_residents(seed):
    c = _random_case(seed)
    keys, B, n0 = c["keys"], c["B"], len(c["keys"])
    kb_out, hint_out, info = BC.next_boundaries(keys, B, c["kb_prev"], c["pos_prev"], c["scount"])
    assert kb_out[0] == 0 and hint_out[0] == 0
    assert np.all(np.diff(hint_out.astype(np.int64)) >= 0)
    assert info["bad"] == (info["disorder"] or info["too_many"] or info["first_empty"] or info["last_empty"])
    if info["bad"]:
        assert np.array_equal(hint_out, np.array([(j * n0) // B for j in range(B)], np.uint32))
        assert np.array_equal(kb_out[1:], keys[hint_out[1:]])
    else:
        assert np.all(np.diff(kb_out.astype(np.int64)) > 0)
        res = np.diff(np.concatenate([hint_out, [n0]]).astype(np.int64))
        assert res.max() <= BC.RESIDENTS_MAX and res[0] > 0 and res[-1] > 0
        # a boundary's place in the list is where its key belongs: behind every smaller key, not behind a larger one
        # (distinct keys, as a walker list has them: between two equal keys there is no key to put a boundary at)
        for j in range(1, B if len(np.unique(keys)) == n0 else 0):
            a = int(hint_out[j])
            assert (a == 0 or keys[a - 1] < kb_out[j]) and (a == n0 or kb_out[j] <= keys[a])
    pos = BC.positions(keys, B, c["kb"])
    assert pos[0] == 0 and pos[B] == n0 and np.all(np.diff(pos.astype(np.int64)) >= 0)


def test_fallback_triggers():
    c = BC.base_case(4000, 3, 1)
    assert BC.next_boundaries(c["keys"], 3, c["kb_prev"], c["pos_prev"], c["scount"])[2]["too_many"]
    c = BC.base_case(900, 3, 1)
    assert not BC.next_boundaries(c["keys"], 3, c["kb_prev"], c["pos_prev"], c["scount"])[2]["bad"]
    for name in ("first_empty", "last_empty"):
        c = CASES[name][0]
        info = BC.next_boundaries(c["keys"], c["B"], c["kb_prev"], c["pos_prev"], c["scount"])[2]
        assert info["bad"] and info[name]
    assert BC._u32_of_double(-1.5) == 0 and BC._u32_of_double(7.9) == 7 and BC._u32_of_double(1e12) == BC.M32


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_meets_its_rule(name):
    c, rules = CASES[name]
    info = BC.next_boundaries(c["keys"], c["B"], c["kb_prev"], c["pos_prev"], c["scount"])[2]
    assert np.all(np.diff(c["keys"].astype(np.int64)) >= 0)
    for r in rules:
        if r == "seams":
            assert {15, 16, 17, 255, 256, 257} <= info["searched"]
        else:
            assert info[r], (name, r, info)
