"""An independent model of the walk's spawn-weight histograms (do_walk.f90:1420-1429, 3295-3311, 3619-3661; gen_hist and
add_to_hist, more_tools.f90:5449-5495): the bin index of x = abs(weight_j)/tau in numpy, the max / min ratio bookkeeping, and the
two printed tables built field by field from the Fortran edit descriptors.  Shares no code with sqmc_amd."""
import math

import numpy as np

NBINS = 10001
LO, HI = 0.0, 10000.0
RATIO_FLOOR = 1e-9          # do_walk.f90:3649


def lbounds():
    """gen_hist(lo=0, hi=10000, nbins=10001): lbounds(i) = lo + (i-1) (hi-lo)/(nbins-1)"""
    return LO + np.arange(NBINS, dtype=np.float64) * ((HI - LO) / (NBINS - 1))


def bin_index(x):
    """ibin = min(nbins, int(1 + (nbins-1)*(x-lbounds(1))/(lbounds(nbins)-lbounds(1)))) evaluated left to right in float64.
    Returns (1-based bins as int64, NaN flags); a NaN has bin 0.  int() of a value past the integer range is undefined in the
    reference: it counts in the last bin."""
    x = np.atleast_1d(np.asarray(x, np.float64))
    nan = np.isnan(x)
    lb = lbounds()
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.float64(NBINS - 1) * (x - lb[0])
        y = y / (lb[NBINS - 1] - lb[0])
        z = np.float64(1.0) + y
    big = ~nan & ~(z < NBINS)
    idx = np.zeros(len(x), np.int64)
    ok = ~nan & ~big
    idx[ok] = np.trunc(z[ok]).astype(np.int64)
    idx[big] = NBINS
    return idx, nan


def histogram(x):
    """(counts[NBINS] with bin b at index b - 1, number of NaNs)"""
    idx, nan = bin_index(x)
    return np.bincount(idx[~nan] - 1, minlength=NBINS).astype(np.int64), int(nan.sum())


def pop(v):
    return bin(int(v)).count("1")


def level_classify(iu, id_, ju, jd):
    """excitation_level (chemistry.f90:7162-7227)"""
    return pop(iu & ~ju) + pop(id_ & ~jd)


def level_ratio(iu, id_, ju, jd, time_sym=False):
    """count_excitations on both spin strings, the smaller of the straight and the spin-swapped count with time_sym (3654-3658)"""
    a = pop(iu & ~ju) + pop(id_ & ~jd)
    return min(a, pop(iu & ~jd) + pop(id_ & ~ju)) if time_sym else a


class Model:
    """what a serial run accumulates from (parent slot, parent, child, weight_j) records"""

    def __init__(self, chem, time_sym=False):
        self.chem, self.ts = chem, time_sym
        self.x, self.hf, self.cls = [], [], []
        self.max_by_level = np.full(8, -1e99)
        self.min_ratio = 1e99

    def add(self, slot, iu, id_, ju, jd, wj, tau):
        x = abs(wj) / tau
        self.x.append(x); self.hf.append(slot == 0)
        lv = level_classify(iu, id_, ju, jd) if (self.chem and wj != 0.0) else 0
        self.cls.append(lv if lv in (1, 2) else 0)
        if x > RATIO_FLOOR:
            l = min(level_ratio(iu, id_, ju, jd, self.ts), 7)
            self.max_by_level[l] = max(self.max_by_level[l], x)
            self.min_ratio = min(self.min_ratio, x)

    def result(self):
        x, hf, cls = np.array(self.x, np.float64), np.array(self.hf, bool), np.array(self.cls)
        mx = float(self.max_by_level.max())
        return dict(bins=histogram(x)[0], bins_hf=histogram(x[hf])[0], bins_single=histogram(x[cls == 1])[0], bins_double=histogram(x[cls == 2])[0],
                    max_ratio_by_level=self.max_by_level.copy(), max_ratio=mx, max_ratio_level=int(np.argmax(self.max_by_level)) if mx > -1e99 else -1,
                    min_ratio=self.min_ratio, n_nan=histogram(x)[1])


# ------------------------------------------------------------------------------------------------ the printed tables
def _i(v, w):
    t = str(int(v)).rjust(w)
    return t if len(t) == w else "*" * w


def _f(v, w, d):
    if v != v:
        return "NaN".rjust(w)
    t = ("%.*f" % (d, v)).rjust(w)
    return t if len(t) == w else "*" * w


def _es(v, w, d):
    if v != v:
        return "NaN".rjust(w)
    if v == 0:
        return ("%.*fE+00" % (d, 0.0)).rjust(w)
    e = int(math.floor(math.log10(abs(v))))
    m = v / 10.0 ** e
    if abs(float("%.*f" % (d, m))) >= 10.0:
        e += 1; m = v / 10.0 ** e
    return ("%.*fE%s%02d" % (d, m, "-" if e < 0 else "+", abs(e))).rjust(w)


def _share(n, tot):
    """float(n)/float(sum): default reals; 0./0. prints NaN"""
    return float("nan") if tot == 0 else float(np.float32(n) / np.float32(tot))


def expected_text(diag, spectral_range=None):
    """do_walk.f90:3295-3320: list-directed headers (a leading blank; an integer(8) in 21 columns), rows '(i5,f10.3,9i11)' and
    '(i5,f10.3,3i11,3f10.6)', the totals '(a,9x,9i11)' and, with spectral_range, the ratio line '(...,9es12.4)'"""
    lb = lbounds()
    hf, sg, db, an = diag["bins_hf"], diag["bins_single"], diag["bins_double"], diag["bins"]
    L = [" Histogram of abs weight multipliers spawned by HF:", " Bin,Lowerbound,Count"]
    for i in range(NBINS):
        L.append(_i(i + 1, 5) + _f(lb[i], 10, 3) + _i(hf[i], 11))
    L.append(" Total=" + _i(int(np.sum(hf)), 21))
    L += [" Histogram of abs weight multipliers spawned by any states:", " Bin,Lowerbound,Singles,Doubles,Total,Singles%,Doubles%,Total%"]
    ts, td, ta = int(np.sum(sg)), int(np.sum(db)), int(np.sum(an))
    for i in range(NBINS):
        L.append(_i(i + 1, 5) + _f(lb[i], 10, 3) + _i(sg[i], 11) + _i(db[i], 11) + _i(an[i], 11)
                 + _f(_share(sg[i], ts), 10, 6) + _f(_share(db[i], td), 10, 6) + _f(_share(an[i], ta), 10, 6))
    L.append("Total=" + " " * 9 + _i(ts, 11) + _i(td, 11) + _i(ta, 11))
    if spectral_range is not None:
        mx, mn = diag["max_ratio"], diag["min_ratio"]
        L.append("Max Ratio, Min Ratio, tau_multiplier, tau for spawning max wt 1=" + _es(mx, 12, 4) + _es(mn, 12, 4) + _es(spectral_range / mx, 12, 4) + _es(1 / mx, 12, 4))
    return "\n".join(L) + "\n"
