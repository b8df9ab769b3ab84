"""An independent model of the energies for extrapolation (energies_for_extrapolation, hci.f90:1824-2017): it imports neither the
library nor the package nor the oracle.  Four parts.

Order.  `shell_sort_magnitude` is shell_sort_real_rank1_int_rank1 (generic_sort.f90:685-735) statement by statement on Python lists,
1-based inside as there: gaps n/2, then gap*5/11 (2 -> 1), an element passes its neighbour only where |neighbour| < |element|, and at
the end the whole list changes sign if its first element is negative.  The sort is not stable; where magnitudes are equal the order
is whatever these statements leave, which is why nothing else can stand in for them.

Sizes.  `truncations(ndets, K)`: batch = ndets // K, i = 1 .. K + 1, kept = min(batch i, ndets), printed = batch i.

Submatrix.  `submatrix(counts, idx, val, sel)`: the principal submatrix on the ascending 0-based rows sel of a matrix in
linalg_checker's storage (diagonal first, then the columns j < i ascending, 1-based), in the same storage.

Lines.  `format_records` writes what the routine prints from a list of records (dictionaries with truncation, state, ndets_printed,
ndets_pt, e_var, pt_big, pt_diff, pt_diff_std_dev, n_connected), edit descriptor by edit descriptor: tN pads to column N, Ew.d has
the form 0.ddE+ee, Fw.d is %w.df.  The list-directed last line of a truncation is written as i12 and es24.16e3."""
from decimal import Decimal

import numpy as np


def shell_sort_magnitude(a):
    """(sorted values, iorder): iorder[k] is the 0-based place in `a` of the k-th sorted element"""
    n = len(a)
    x = [None] + [float(v) for v in a]                # 1-based, as the Fortran
    o = [None] + list(range(n))
    inc = n // 2
    while inc > 0:
        for i in range(inc + 1, n + 1):
            j = i
            t, ti = x[i], o[i]
            while j >= inc + 1:
                if abs(x[j - inc]) >= abs(t):
                    break
                x[j] = x[j - inc]; o[j] = o[j - inc]
                j -= inc
            x[j] = t; o[j] = ti
        inc = 1 if inc == 2 else inc * 5 // 11
    if n and x[1] < 0:
        x = [None] + [-v for v in x[1:]]
    return x[1:], o[1:]


def truncations(ndets, k):
    batch = ndets // k
    return [(min(batch * i, ndets), batch * i) for i in range(1, k + 2)]


def submatrix(counts, idx, val, sel):
    counts = np.asarray(counts, np.int64); idx = np.asarray(idx, np.int64); val = np.asarray(val, np.float64)
    sel = [int(s) for s in sel]
    assert all(b > a for a, b in zip(sel, sel[1:])) and (not sel or (sel[0] >= 0 and sel[-1] < len(counts)))
    new = {s: k for k, s in enumerate(sel)}
    start = np.concatenate(([0], np.cumsum(counts)))
    oc, oi, ov = [], [], []
    for s in sel:
        kept = 0
        for q in range(int(start[s]), int(start[s + 1])):
            j = int(idx[q]) - 1
            if j in new:
                oi.append(new[j] + 1); ov.append(float(val[q])); kept += 1
        oc.append(kept)
    return np.array(oc, np.int64), np.array(oi, np.int64), np.array(ov, np.float64)


# ------------------------------------------------------------------------------------------------------------------- the lines
def _f(x, w, d):
    s = "%.*f" % (d, x)
    return s.rjust(w)


def _e(x, w, d):
    """Ew.d: 0.d1..dd E+ee, the value rounded to d significant digits"""
    if x == 0:
        return ("0." + "0" * d + "E+00").rjust(w)
    v = Decimal(repr(abs(float(x))))
    ex = v.adjusted() + 1                               # v = 0.ddd x 10^ex
    digits = int((v.scaleb(d - ex)).quantize(Decimal(1), rounding="ROUND_HALF_EVEN"))
    if digits == 10 ** d:                               # rounded up to 1.00: 0.10 x 10^(ex + 1)
        digits //= 10; ex += 1
    return ("%s0.%0*dE%s%02d" % ("-" if x < 0 else "", d, digits, "-" if ex < 0 else "+", abs(ex))).rjust(w)


def _tab(s, col):
    return s.ljust(col - 1)


def _es24(x):
    m, e = ("%.16e" % x).split("e")
    return ("%sE%s%03d" % (m, "-" if int(e) < 0 else "+", abs(int(e)))).rjust(24)


SORTING = "Sorting global dets list to create truncated wavefunctions"
TO_DETS = "Converting to determinant basis"
NO_MORE = "From now on, no more time-reversal symmetry"


def format_state(r, eps_var, eps_pt):
    i, e, big, diff, sd = r["state"], r["e_var"], r["pt_big"], r["pt_diff"], r["pt_diff_std_dev"]
    long_head = "eps_var, eps_pt, ndets, ndets_connected(total), Variational, PT_actv, PT_full, Total Energies(%1d)=" % i
    long_head += _e(eps_var, 9, 2) + _e(eps_pt, 9, 2) + "%9d%11d" % (r["ndets_printed"], r["n_connected"])
    out = ["", "State%4d:" % i, _tab("Variational energy(%1d)=" % i, 36) + _f(e, 15, 9)]
    if sd == 0.0:
        out.append(_tab("2nd-order PT energy lowering(%1d)=" % i, 36) + _f(big, 15, 9))
        out.append(_tab("Total energy(%2d)=" % i, 36) + _f(e + big, 15, 9))
        out.append(long_head + _f(e, 16, 9) + _f(big, 15, 9) + _f(big, 15, 9) + _f(e + big, 16, 9))
    else:
        out.append(_tab("2nd-order PT energy lowering(%1d)=" % i, 36) + _f(big + diff, 15, 9) + " +-" + _f(sd, 12, 9) + " (" + _f(big, 13, 9) + _f(diff, 13, 9) + ")")
        out.append(_tab("Total energy(%1d)=" % i, 36) + _f(e + big + diff, 15, 9) + " +-" + _f(sd, 12, 9))
        out.append(long_head + _f(e, 16, 9) + _f(big + diff, 15, 9) + _f(big + diff, 15, 9) + _f(e + big + diff, 16, 9) + " +-" + _f(sd, 12, 9))
    return out


def format_records(records, eps_var, eps_pt, time_sym):
    """every line of the routine for deterministic PT stages, in order: the heading, then per truncation the two time-symmetry lines
    where they apply, the states' lines and the ndets / energy line"""
    out = ["", SORTING]
    trunc = sorted(set(r["truncation"] for r in records))
    for t in trunc:
        rs = sorted((r for r in records if r["truncation"] == t), key=lambda r: r["state"])
        if time_sym:
            out += ["", TO_DETS, NO_MORE, ""]
        for r in rs:
            out += format_state(r, eps_var, eps_pt)
        out.append(" ndets: %12d energy: %s" % (rs[0]["ndets_pt"], _es24(rs[0]["e_var"])))
    return out
