"""The inputs of tests/test_gpu_gap_sort.py, checked on the CPU: every case holds, in the bucket it aims at, what it is named for
(gap_sort_cases.check_case: spawns per gap, distinct keys, creation order, words per partition row -- all derived from the
equal-residents boundary rule, not from how the case was written), and the set covers what the sort can meet."""
import json

import pytest

import gap_sort_cases as GS


@pytest.fixture(scope="module")
def prepared(oracle, c2_walk, c2_setup, tmp_path_factory):
    return GS.prepared(c2_walk, c2_setup, tmp_path_factory)


def test_every_case_holds_what_it_is_named_for(prepared):
    kc = prepared["kc"]
    A = kc["A"]
    f = {c["name"]: GS.check_case(c, kc) for c in prepared["cases"]}
    assert f["S_0"]["S"] == 0 and f["S_1"]["S"] == 1
    assert list(f["only_gap_0"]["per_gap"]) == [0] and list(f["only_gap_R"]["per_gap"]) == [f["only_gap_R"]["R"]]
    for how in ("descending", "interleaved"):
        assert max(f["distinct_keys_in_one_gap_" + how]["keys_per_gap"].values()) >= 5
    for n in (65, A + 1, 1000):
        assert max(f["one_determinant_%d_spawns" % n]["per_gap"].values()) >= n
    assert f["one_determinant_%d_spawns" % (A + 1)]["S"] > A and f["one_determinant_65_spawns"]["S"] > 64
    g = f["heavy_gap_among_empty_gaps"]
    assert g["S"] >= 200 and len(g["per_gap"]) == 1 and g["R"] >= 500
    w = f["wide_resident_list"]
    assert kc["GAP_SORT_MAX_R"] < w["R"] <= kc["CAP_R"] and 0 < w["S"] < 32
    assert len(prepared["cases"]) == 11
    print(json.dumps({k: dict(B=v["B"], R=v["R"], S=v["S"], per_gap=v["per_gap"], rows=v["rows"]) for k, v in f.items()}))
