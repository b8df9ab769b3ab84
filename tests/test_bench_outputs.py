"""bench.py --dump-outputs: what it writes for a walker list, checked on a stand-in for the library context (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Walkers:
    """download_walkers() of a list of n walkers with 64-bit determinants"""
    def __init__(self, n):
        r = np.random.default_rng(3)
        self.w = dict(up=r.integers(0, 2**64, n, dtype=np.uint64), dn=r.integers(0, 2**64, n, dtype=np.uint64), wt=r.normal(size=n),
                      imp_distance=r.integers(0, 3, n).astype(np.int8), initiator=r.integers(0, 4, n).astype(np.int8),
                      matrix_elements=r.normal(size=n), e_num=r.normal(size=n), e_den=r.normal(size=n))

    def download_walkers(self):
        return self.w


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _dets(halves):
    return (halves[:, 0].astype(np.uint64) << np.uint64(32)) | halves[:, 1].astype(np.uint64)


def test_dump_is_exact_and_complete_under_the_budget(tmp_path):
    g = _Walkers(5000)
    bench.dump_outputs(str(tmp_path), np.arange(16.0), g, 0, 1)
    out = _load(str(tmp_path))
    assert set(out) == {"step_sums", "walkers_up", "walkers_dn", "walkers_wt", "walkers_matrix_elements", "walkers_e_num", "walkers_e_den",
                        "walkers_imp_distance", "walkers_initiator"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["step_sums"], np.arange(16.0))
    assert np.array_equal(_dets(out["walkers_up"]), g.w["up"]) and np.array_equal(_dets(out["walkers_dn"]), g.w["dn"])
    assert np.array_equal(out["walkers_wt"], g.w["wt"]) and np.array_equal(out["walkers_initiator"], g.w["initiator"])


def test_dump_of_a_long_list_is_a_fixed_sample_within_64_mb(tmp_path):
    g = _Walkers(1_200_000)
    for d, rank, world in (("a", 0, 1), ("b", 0, 1), ("r0", 0, 2), ("r1", 1, 2)):
        bench.dump_outputs(str(tmp_path / d), np.zeros(16), g, rank, world)
    size = lambda d: sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    assert size(str(tmp_path / "a")) <= 64 << 20
    assert size(str(tmp_path / "r0")) + size(str(tmp_path / "r1")) <= 64 << 20
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[k], b[k]) for k in a)                  # the same rows every time
    up = _dets(a["walkers_up"])
    assert 0 < len(up) < 1_200_000
    rows = np.searchsorted(np.sort(g.w["up"]), up)                      # a sample of the list's rows, in list order
    assert np.array_equal(np.sort(g.w["up"])[rows], up)
    assert "walkers_up_rank1" in _load(str(tmp_path / "r1"))
