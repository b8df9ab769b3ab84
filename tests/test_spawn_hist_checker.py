"""The checker of the spawn-weight histograms (tests/spawn_hist_checker.py) on its own, and sqmc_amd.host.format_spawn_histograms
against it: bin edges, field widths, NaN where a column sum is 0.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import spawn_hist_checker as SH          # noqa: E402


def test_bin_edges():
    below_one = np.nextafter(1.0, 0.0)
    x = np.array([0.0, below_one, 1.0, 9999.5, 10000.0, 1e300, np.nan, np.inf, np.nextafter(10000.0, 0.0), 2.0 ** 31, 12.0])
    idx, nan = SH.bin_index(x)
    assert idx.tolist() == [1, 1, 2, 10000, 10001, 10001, 0, 10001, 10000, 10001, 13]
    assert nan.tolist() == [False] * 6 + [True] + [False] * 4
    h, n_nan = SH.histogram(x)
    assert n_nan == 1 and h.sum() == len(x) - 1 and h[0] == 2 and h[1] == 1 and h[9999] == 2 and h[10000] == 4 and h[12] == 1
    lb = SH.lbounds()
    assert lb[0] == 0.0 and lb[1] == 1.0 and lb[10000] == 10000.0 and len(lb) == SH.NBINS          # unit-wide bins


def test_model_levels_and_ratios():
    m = SH.Model(chem=True)
    m.add(0, 0b0111, 0b0111, 0b1011, 0b0111, -0.004, 0.002)          # single from slot 0: x = 2
    m.add(1, 0b0111, 0b0111, 0b1011, 0b1011, 0.05, 0.002)            # double: x = 25
    m.add(1, 0b0111, 0b0111, 0b0111, 0b0111, 0.0, 0.002)             # no move
    r = m.result()
    assert r["bins"][2] == 1 and r["bins"][25] == 1 and r["bins"][0] == 1 and r["bins"].sum() == 3
    assert r["bins_hf"].sum() == 1 and r["bins_hf"][2] == 1
    assert r["bins_single"].sum() == 1 and r["bins_double"].sum() == 1 and r["bins_double"][25] == 1
    assert r["max_ratio"] == 25.0 and r["max_ratio_level"] == 2 and r["min_ratio"] == 2.0 and r["max_ratio_by_level"][1] == 2.0
    ts = SH.Model(chem=True, time_sym=True)
    ts.add(0, 0b0011, 0b0101, 0b0101, 0b0011, 0.01, 0.01)             # the spin-swapped child: level 0, not 2
    assert ts.result()["max_ratio_level"] == 0


def _diag(chem):
    rng = np.random.default_rng(4)
    d = {k: np.zeros(SH.NBINS, np.int64) for k in ("bins", "bins_hf", "bins_single", "bins_double")}
    d["bins"][[0, 3, 17, 10000]] = [12345678901, 7, 1, 2]
    d["bins_hf"][[0, 3]] = [40, 2]
    if chem:
        d["bins_single"][[3, 17]] = [5, 1]
        d["bins_double"][[3, 10000]] = [2, 2]
    d.update(nbins=SH.NBINS, max_ratio=12345.678, min_ratio=3.25e-4, max_ratio_level=2, max_ratio_by_level=np.full(8, -1e99), n_nan=0)
    return d


def test_field_widths_of_a_hand_made_histogram():
    from sqmc_amd.host import format_spawn_histograms
    d = _diag(True)
    want = SH.expected_text(d, spectral_range=41.5)
    got = format_spawn_histograms(d, True, spectral_range=41.5)
    assert got == want
    lines = got.split("\n")
    assert len(lines) == 2 * SH.NBINS + 8 and lines[-1] == ""
    assert lines[2] == "    1     0.000         40" and len(lines[2]) == 26                       # (i5,f10.3,9i11)
    assert lines[2 + 10000] == "10001 10000.000          0"
    assert lines[2 + SH.NBINS] == " Total=" + "42".rjust(21)
    row = lines[5 + SH.NBINS + 3]
    assert len(row) == 5 + 10 + 33 + 30 and row == "    4     3.000          5          2          7  0.833333  0.500000  0.000000"          # (i5,f10.3,3i11,3f10.6)
    assert lines[5 + SH.NBINS] == "    1     0.000          0          012345678901  0.000000  0.000000  1.000000"          # a count that fills i11
    assert lines[-3] == "Total=" + " " * 9 + "          6          412345678911"                  # (a,9x,9i11)
    assert lines[-2] == "Max Ratio, Min Ratio, tau_multiplier, tau for spawning max wt 1=  1.2346E+04  3.2500E-04  3.3615E-03  8.1000E-05"
    assert format_spawn_histograms(d, True) == SH.expected_text(d)                                # without the ratio line
    d["bins"][5] = 10 ** 11                                                                        # a count that does not fit i11
    assert format_spawn_histograms(d, True).split("\n")[5 + SH.NBINS + 5][37:48] == "*" * 11


def test_nan_where_a_column_sum_is_zero():
    from sqmc_amd.host import format_spawn_histograms
    d = _diag(False)
    got = format_spawn_histograms(d, False)
    assert got == SH.expected_text(d)
    row = got.split("\n")[5 + SH.NBINS + 3]
    assert row == "    4     3.000          0          0          7       NaN       NaN  0.000000"
    assert got.count("       NaN       NaN") == SH.NBINS


def test_percentages_divide_in_single_precision():
    """float(n)/float(sum) is a quotient of default reals, itself rounded to single: 27/29 and 16/51 print 0.931035 and 0.313726, where
    the double-precision quotient of the same two singles prints 0.931034 and 0.313725"""
    from sqmc_amd.host import format_spawn_histograms
    d = {k: np.zeros(SH.NBINS, np.int64) for k in ("bins", "bins_hf", "bins_single", "bins_double")}
    d["bins"][[2, 4, 6]] = [27 + 16, 2, 35]
    d["bins_single"][[2, 4]] = [27, 2]
    d["bins_double"][[2, 6]] = [16, 35]
    d.update(nbins=SH.NBINS, max_ratio=6.5, min_ratio=2.5, max_ratio_level=2, max_ratio_by_level=np.full(8, -1e99), n_nan=0)
    got = format_spawn_histograms(d, True)
    assert got == SH.expected_text(d)
    assert "%.6f %.6f" % (27 / 29, 16 / 51) == "0.931034 0.313725"
    assert got.split("\n")[5 + SH.NBINS + 2] == "    3     2.000         27         16         43  0.931035  0.313726  0.537500"
