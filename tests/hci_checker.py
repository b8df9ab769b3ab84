"""An independent, brute-force reference for Heat-bath CI connection generation and the Epstein-Nesbet sum, on top of
tests/proposal_checker.py: every raw single and double excitation of a source determinant with its element from second
quantisation, screened one by one, merged in a dictionary.  Nothing here comes from oracle/ or from the HIP library; no heat-bath
table is walked and no Slater-Condon rule is used.

What the generator is, read from the reference (find_important_connected_dets_chem, chemistry.f90:6819-7159;
find_important_connected_dets_heg, heg.f90:2475-2727; find_doubly_excited, semistoch.f90:1750-2131):

  * source i with coefficient c_i is screened with eps_i = eps / |c_i|; slot 0 of its list is the source itself with element 0
    (chemistry.f90:6893-6896) and e_mix_den = c_i (semistoch.f90:2062-2063);
  * a single excitation is dropped when |H| < eps_i (chemistry.f90:6956: a tie is KEPT), a chemistry double when its |H| <= eps_i
    (:7042: a tie is DROPPED; no double at all when eps_i > max_double, :6995), a HEG double when |H| <= eps_i (heg.f90:2608, 2629:
    DROPPED).  H is the raw element between the two determinants as written, before any time-reversal factor;
  * with time-reversal symmetry (chemistry.f90:6949-6952, 6961-6971, 7110-7132) an excitation is skipped when new_up == new_dn and
    z < 0 and when it is the time-reversed partner of the source; the kept element is multiplied by 1/sqrt(2) when the source has
    up == dn and the new determinant has not, by sqrt(2) the other way round, and a new determinant with up > dn is swapped to its
    representative with a factor z.  Two raw excitations of one source may reach one representative: the merge adds them;
  * the active-space masks act on the new determinant before that swap (:6926-6947, 7087-7108);
  * a source with c_i == 0 is never handed to the generator (the guards at semistoch.f90:1762, 1798, 1854, 1891): it gives no
    connection and no slot of its own.  (The reference then re-reads the buffers of the previous source with a factor c_i = 0, which
    adds zeros to sums that exist already; what is defined is: nothing from this source.)

A path whose | |H c| / eps - 1 | <= BORDERLINE is *borderline*: the checker does not decide it, it lists it, and compare() refuses
a case that has one.  A path whose |H| does not exceed its own rounding bound is *noise* (a zero that second quantisation did not
cancel exactly): it may or may not be present, with a value inside its bound."""
import math

from tests import proposal_checker as PC

BORDERLINE = 1e-9
U = 2.0 ** -53
SQRT2 = math.sqrt(2.0)

SINGLE, DOUBLE, HEG = "single", "double", "heg"
KEEPS_TIE = {SINGLE: True, DOUBLE: False, HEG: False}

_ROWS = {}


class Path:
    """one raw excitation of a source: det = where it lands (the representative under time symmetry), new = the determinant as
    excited, raw = <new|H|source> (what is screened), value = raw with the time-reversal factors; n, s = number of terms, sum|terms|"""
    __slots__ = ("det", "new", "cls", "raw", "value", "n", "s")

    def __init__(self, det, new, cls, raw, value, n, s):
        self.det, self.new, self.cls, self.raw, self.value, self.n, self.s = det, new, cls, raw, value, n, s

    @property
    def noise(self):
        return abs(self.raw) <= PC.rounding_bound(self.n, self.s)

    def bound(self, c):
        """|kernel's value * c - ours|: the element's own bound, scaled, + the products with the factor and with c"""
        scale = abs(self.value / self.raw) if self.raw != 0.0 else 1.0
        return (PC.rounding_bound(self.n, self.s) * scale + 4.0 * U * abs(self.value)) * abs(c)


def _excitation_class(source, new):
    return SINGLE if PC._pop(source[0] & ~new[0]) + PC._pop(source[1] & ~new[1]) == 1 else DOUBLE


def raw_paths(H, source, time_sym=False, z=1):
    """every raw single and double excitation of |up, dn> as given whose element has at least one term, in a fixed order"""
    key = (id(H), tuple(source), bool(time_sym), z)
    if key in _ROWS:
        return _ROWS[key]
    up, dn = int(source[0]), int(source[1])
    heg = isinstance(H, PC.HegH)
    assert not (heg and time_sym)
    out = []
    for nu, nd in (PC.excitations_heg(H, up, dn) if heg else PC.excitations_chem(up, dn, H.norb)):
        if time_sym:
            if nu == nd and z < 0:
                continue
            if up == nd and dn == nu:
                continue
        raw, n, s = H.element(up, dn, nu, nd)
        if n == 0:
            continue
        value, det = raw, (nu, nd)
        if time_sym:
            if up == dn and nu != nd:
                value = value / SQRT2
            if nu == nd and up != dn:
                value = value * SQRT2
            if nu > nd:
                det, value = (nd, nu), z * value
        out.append(Path(det, (nu, nd), HEG if heg else _excitation_class((up, dn), (nu, nd)), raw, value, n, s))
    _ROWS[key] = out
    return out


def diagonal(H, det, time_sym=False, z=1):
    return H.element_ts(det[0], det[1], det[0], det[1], z) if time_sym else H.element(det[0], det[1], det[0], det[1])


def in_active_space(new, core_up, core_dn, virt_up, virt_dn):
    return (new[0] & core_up) == core_up and (new[1] & core_dn) == core_dn and not (new[0] & virt_up) and not (new[1] & virt_dn)


class Connections:
    """merged: det -> (num, den); bound: det -> error bound on num; exact_zero: dets whose num is exactly 0.0 (a self slot that nothing
    else reaches, diag_mode 0); raw: [(det, source index, num, bound)] in source order, the self slot first; optional: dets that only
    noise paths reach; borderline: [(source index, det, |H c| / eps)]; noise_bound: det -> sum of the noise paths' bounds; noise_paths: (source index, det) ->
    those bounds one by one"""

    def __init__(self):
        self.merged, self.bound, self.exact_zero, self.raw, self.optional, self.borderline = {}, {}, set(), [], set(), []
        self.parts, self.noise_paths, self.worst_at = {}, {}, None          # worst_at: where compare() found its worst ratio


def connections(H, sources, coeffs, eps, diag_mode=0, active_space=None, slice_of=None, time_sym=False, z=1, threshold=None):
    """active_space = (core_up, core_dn, virt_up, virt_dn, mode) with mode 0 / 1 (inside only) / 2 (outside only); slice_of(det) ->
    bool keeps the determinants of one slice (the self slots too); threshold(c) -> eps_i replaces eps / |c| (for doctored results)"""
    out = Connections()
    parts, noise_only = {}, {}
    for i, (src, c) in enumerate(zip(sources, coeffs)):
        src, c = (int(src[0]), int(src[1])), float(c)
        if c == 0.0:
            continue
        eps_i = threshold(c) if threshold else eps / abs(c)
        items = []
        if diag_mode == 1:
            h, n, s = diagonal(H, src, time_sym, z)
            items.append((src, h * c, (PC.rounding_bound(n, s) + 2.0 * U * abs(h)) * abs(c), c, False))
        else:
            items.append((src, 0.0, 0.0, c, False))
        for p in raw_paths(H, src, time_sym, z):
            if active_space is not None and active_space[4]:
                inside = in_active_space(p.new, *active_space[:4])
                if inside != (active_space[4] == 1):
                    continue
            if p.noise:
                if abs(p.raw) + PC.rounding_bound(p.n, p.s) >= eps_i:       # could pass the screen as computed in another order
                    items.append((p.det, p.value * c, p.bound(c), 0.0, True))
                continue
            ratio = abs(p.raw) / eps_i if eps_i > 0 else math.inf
            if abs(ratio - 1.0) <= BORDERLINE:
                out.borderline.append((i, p.det, ratio))
                continue
            if ratio < 1.0:
                continue
            items.append((p.det, p.value * c, p.bound(c), 0.0, False))
        for k, (det, num, b, den, noise) in enumerate(items):
            if slice_of is not None and not slice_of(det):
                continue
            if noise:
                noise_only.setdefault(det, []).append(b + abs(num))
                out.noise_paths.setdefault((i, det), []).append(b + abs(num))
                continue
            parts.setdefault(det, []).append((num, b, den, k == 0))
            out.raw.append((det, i, num, b))
    for det, lst in parts.items():
        num = math.fsum(x[0] for x in lst)
        den = math.fsum(x[2] for x in lst)
        b = math.fsum(x[1] for x in lst) + max(len(lst) - 1, 0) * U * math.fsum(abs(x[0]) for x in lst)
        b += math.fsum(noise_only.get(det, []))
        out.merged[det], out.bound[det] = (num, den), b
        if all(x[3] for x in lst) and diag_mode != 1 and det not in noise_only:
            out.exact_zero.add(det)
    out.optional = {d for d in noise_only if d not in parts}
    out.noise_bound = {d: math.fsum(v) for d, v in noise_only.items()}
    out.parts = parts
    return out


def compare(exp, up, dn, num, den, diag_mode=0):
    """the door's output (merged modes 0 and 1: arrays sorted by (up, dn); mode 2: generation order, den = source index) against
    the checker's Connections.  Returns (failures, worst |delta| / bound)."""
    fails, worst = [], 0.0
    up, dn, num, den = [int(x) for x in up], [int(x) for x in dn], [float(x) for x in num], [float(x) for x in den]
    if exp.borderline:
        return [("borderline", "%d paths sit on the threshold, e.g. %s" % (len(exp.borderline), exp.borderline[:3]))], 0.0
    if diag_mode == 2:
        return _compare_raw(exp, up, dn, num, den)
    keys = list(zip(up, dn))
    if any(a >= b for a, b in zip(keys, keys[1:])):
        fails.append(("order", "not strictly increasing in (up, dn): a determinant is repeated or out of place"))
    got = {}
    for k, x, y in zip(keys, num, den):
        got.setdefault(k, (x, y))
    missing = [k for k in exp.merged if k not in got]
    extra = [k for k in got if k not in exp.merged and k not in exp.optional]
    if missing:
        fails.append(("set", "%d determinants missing, e.g. %s" % (len(missing), [tuple(map(hex, k)) for k in missing[:3]])))
    if extra:
        fails.append(("set", "%d determinants too many, e.g. %s" % (len(extra), [tuple(map(hex, k)) for k in extra[:3]])))
    for k, (x, y) in got.items():
        if k in exp.merged:
            want, wden = exp.merged[k]
            b = exp.bound[k]
            if y != wden:
                fails.append(("den", "%s: e_mix_den %r, expected %r" % (tuple(map(hex, k)), y, wden)))
            if k in exp.exact_zero:
                if x != 0.0:
                    fails.append(("num", "%s: a bare self slot carries %r" % (tuple(map(hex, k)), x)))
                continue
        elif k in exp.optional:
            want, b = 0.0, exp.noise_bound[k]
            if y != 0.0:
                fails.append(("den", "%s: e_mix_den %r on a connection" % (tuple(map(hex, k)), y)))
        else:
            continue
        d = abs(x - want)
        if not d <= b:
            fails.append(("num", "%s: %r against %r, bound %.3g" % (tuple(map(hex, k)), x, want, b)))
        if b > 0 and d / b > worst:
            worst, exp.worst_at = d / b, k
    return fails, worst


def _compare_raw(exp, up, dn, num, src):
    """raw mode: per source index the multiset of generated determinants, the self slot in front, every value within its bound"""
    fails, worst = [], 0.0
    got, want = {}, {}
    for k, (u, d, x, s) in enumerate(zip(up, dn, num, src)):
        if s != int(s):
            fails.append(("source", "entry %d: source index %r" % (k, s)))
            continue
        got.setdefault(int(s), []).append(((u, d), x))
    for det, i, x, b in exp.raw:
        want.setdefault(i, []).append((det, x, b))
    if sorted(got) != sorted(want):
        fails.append(("source", "sources with output %s, expected %s" % (sorted(got)[:8], sorted(want)[:8])))
    if [int(s) for s in src] != sorted(int(s) for s in src):
        fails.append(("order", "raw output is not in source order"))
    for i in sorted(set(got) & set(want)):
        g, w = got[i], want[i]
        if g[0][0] != w[0][0]:
            fails.append(("self", "source %d: first entry %s is not the source" % (i, g[0][0])))
            continue
        gd, wd = {}, {}
        for det, x in g[1:]:
            gd.setdefault(det, []).append(x)
        for det, x, b in w[1:]:
            wd.setdefault(det, []).append((x, b))
        gd.setdefault(g[0][0], []).insert(0, g[0][1]); wd.setdefault(w[0][0], []).insert(0, (w[0][1], w[0][2]))
        lost = sorted(k for k in wd if len(gd.get(k, [])) < len(wd[k]))
        more = sorted(k for k in gd if len(gd[k]) - len(wd.get(k, [])) > len(exp.noise_paths.get((i, k), [])))
        if lost or more:
            fails.append(("set", "source %d: not generated %s, generated and not expected %s" % (
                i, [tuple(map(hex, k)) for k in lost[:3]], [tuple(map(hex, k)) for k in more[:3]])))
            continue
        for det, xs in gd.items():
            ws = sorted(wd.get(det, []))
            noise = sorted(exp.noise_paths.get((i, det), []))
            xs = sorted(xs, key=abs)
            extra, xs = xs[:len(xs) - len(ws)], sorted(xs[len(xs) - len(ws):])
            if any(not abs(x) <= nb for x, nb in zip(extra, reversed(noise))):
                fails.append(("num", "source %d -> %s: %r where the element is zero within rounding" % (i, tuple(map(hex, det)), extra)))
            for x, (y, b) in zip(xs, ws):
                d = abs(x - y)
                if not d <= b:
                    fails.append(("num", "source %d -> %s: %r against %r, bound %.3g" % (i, tuple(map(hex, det)), x, y, b)))
                if b > 0 and d / b > worst:
                    worst, exp.worst_at = d / b, det
    return fails, worst


def pt2(H, var, coeffs, e_var, eps, time_sym=False, z=1):
    """brute-force Epstein-Nesbet: sum over the connected determinants a outside var of (sum_i H_ai c_i)^2 / (E_var - H_aa).
    Returns (delta_e, determinants outside, determinants visited (the merged list, var's own slots included), bound, borderline)"""
    var = [(int(a), int(b)) for a, b in var]
    con = connections(H, var, coeffs, eps, 0, time_sym=time_sym, z=z)
    inside = set(var)
    terms, bounds = [], []
    for det, (x, _) in con.merged.items():
        if det in inside:
            continue
        haa, n, s = diagonal(H, det, time_sym, z)
        den = e_var - haa
        t = x * x / den
        bx, bd = con.bound[det], PC.rounding_bound(n, s) + U * (abs(e_var) + abs(haa))
        terms.append(t)
        bounds.append((2.0 * abs(x) * bx + bx * bx) / abs(den) + abs(t) * (bd / abs(den) + 3.0 * U))
    n_out = len(terms)
    bound = math.fsum(bounds) + n_out * U * math.fsum(abs(t) for t in terms)
    return math.fsum(terms), n_out, len(con.merged), bound, con.borderline


def screen_values(H, sources, coeffs, time_sym=False, z=1):
    """|H c| of every live path of every source: what pick_eps chooses between"""
    vals = []
    for src, c in zip(sources, coeffs):
        if c != 0.0:
            vals += [abs(p.raw * c) for p in raw_paths(H, (int(src[0]), int(src[1])), time_sym, z) if not p.noise]
    return vals


def pick_eps(values, k, min_gap=1e-6):
    """the geometric midpoint between the k-th and the (k+1)-th largest distinct value (k is moved up to the next pair that lies
    at least min_gap apart, relatively): a threshold that keeps the k largest and sits far from every element"""
    v = sorted({abs(float(x)) for x in values if x != 0.0}, reverse=True)
    assert 1 <= k < len(v), (k, len(v))
    while k < len(v) and not v[k - 1] > v[k] * (1.0 + min_gap):
        k += 1
    assert k < len(v)
    return math.sqrt(v[k - 1] * v[k])


# ---------------------------------------------------------------------------------------------- determinant keys and slices
def colex_rank(det):
    return sum(math.comb(p, i + 1) for i, p in enumerate(PC._bits(det)))


def det_key(det, norb, ndn):
    """rank of the up string times C(norb, ndn) plus the rank of the dn string: the order of (up, dn) as integers"""
    return colex_rank(det[0]) * math.comb(norb, ndn) + colex_rank(det[1])


def key_space(norb, nup, ndn):
    """invalid_key + 1 = 2^bits, bits the smallest with 2^bits - 1 >= the number of determinants"""
    total, bits = math.comb(norb, nup) * math.comb(norb, ndn), 1
    while (1 << bits) - 1 < total:
        bits += 1
    return 1 << bits


def slice_index(det, norb, nup, ndn, n_slices):
    """the slice of n_slices equal parts of [0, invalid_key] that holds det: slice s is [floor(s span), floor((s+1) span)) with
    span = (invalid_key + 1) / n_slices, the last one open above"""
    k, space = det_key(det, norb, ndn), key_space(norb, nup, ndn)
    s = min(k * n_slices // space, n_slices - 1)
    while s + 1 < n_slices and k >= (space * (s + 1)) // n_slices:
        s += 1
    while s > 0 and k < (space * s) // n_slices:
        s -= 1
    return s
