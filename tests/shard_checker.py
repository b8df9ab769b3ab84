"""An independent model of the phases of the sharded (multi-rank) step, CPU only.

Written from include/sqmc_gpu.h -- the "upper triangular" storage of the projector, the three phases sqmc_gpu_shard_begin /
_pack / _finish, the 32-byte wire record, out_stats -- and from the comment above djb_hash128 in sqmc_amd/csrc/walk_kernels.h.
Nothing here imports oracle/ or sqmc_amd, and nothing restates a kernel: rows are Python lists, sums are fractions.Fraction
or math.fsum, the hash is Python's unbounded integers reduced by hand, routing is a list comprehension per destination.

  expand_upper   the symmetric matrix from its upper storage, as rows of (col, val)
  project        w_i + sum_k A_ik x_k + e_trial tau x_i for chosen rows, exactly (Fraction) or with a rounding bound
  gather         a rank's share of the deterministic weights in the global vector, zeros elsewhere
  owner_djb      the reference's get_det_owner -> hash -> djb_hash in big integers
  route          stable partition of spawn records by owner, weight-0 records dropped
  encode/decode  the wire record {up, dn, weight bits, flags}
  conservation   nwalk_before_merge and w_abs_before_merge of a finish against what went in
The finish itself (merge, rounding, reweighting, sums) is anneal_checker.fold / anneal_checker.sums, unchanged.

Three deliberate mistakes can be switched on (drop_last_at_64, rows_as_local, unstable): tests/test_shard_checker.py shows
that the comparison functions below, the ones tests/shard_phase_cases.py judges the library with, report each of them."""
import math
import struct
from fractions import Fraction

import numpy as np

from proposal_checker import rounding_bound

SEAM_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 193)


# ------------------------------------------------------------------------------------------------ the projector
def expand_upper(counts, indices, values):
    """include/sqmc_gpu.h: row_counts(n), 1-based column indices, values; "every stored (i,m) with i != m is applied to both
    y(i) and y(m)".  So a stored (i, m, v) is the element A_im = v and, off the diagonal, also A_mi = v.
    Returns the full rows: rows[i] = [(col, val), ...] by increasing column (0-based)."""
    n = len(counts)
    rows = [[] for _ in range(n)]
    k = 0
    for i in range(n):
        for _ in range(int(counts[i])):
            m, v = int(indices[k]) - 1, float(values[k])
            k += 1
            assert 0 <= m < n, "column %d of row %d is outside the matrix" % (m + 1, i + 1)
            rows[i].append((m, v))
            if m != i:
                rows[m].append((i, v))
    assert k == len(values) == len(indices), "sum(row_counts) is not the number of stored elements"
    return [sorted(r, key=lambda cv: cv[0]) for r in rows]


def is_exact_double(q):
    """does the Fraction q convert to a double without rounding?"""
    return Fraction(float(q)) == q


def project(rows, x, e_trial, tau, exact, only=None, drop_last_at_64=False):
    """y_i = x_i + sum_k A_ik x_k + e_trial tau x_i for the rows in `only` (default: all), x the all-reduced vector of the
    deterministic weights (x_i = w_i on the row's owner).
    exact=True: list of Fractions.  exact=False: (list of doubles by math.fsum of the rounded terms, list of bounds) with
    bound_i = rounding_bound(n_terms + 2, sum |terms|): the n_terms products of the row, the walker's own weight and the
    e_trial term, each a product or two, added in any order.
    drop_last_at_64: the planted mistake -- a row whose length is a multiple of 64 loses its last term."""
    only = range(len(rows)) if only is None else only
    if exact:
        et = Fraction(e_trial) * Fraction(tau)
        out = []
        for i in only:
            r = rows[i][:-1] if (drop_last_at_64 and len(rows[i]) and len(rows[i]) % 64 == 0) else rows[i]
            out.append(Fraction(x[i]) + sum((Fraction(v) * Fraction(x[c]) for c, v in r), Fraction(0)) + et * Fraction(x[i]))
        return out
    ys, bounds = [], []
    for i in only:
        r = rows[i][:-1] if (drop_last_at_64 and len(rows[i]) and len(rows[i]) % 64 == 0) else rows[i]
        terms = [float(x[i])] + [v * float(x[c]) for c, v in r] + [e_trial * tau * float(x[i])]
        ys.append(math.fsum(terms))
        bounds.append(rounding_bound(len(r) + 2, math.fsum(abs(t) for t in terms)))
    return ys, bounds


def gather(local_weights, global_rows, n_imp, rows_as_local=False):
    """x[g_k] = w_k for the k-th deterministic walker a rank owns, 0 on every other rank's rows: the vectors of the ranks
    have disjoint support, so their sum (the all-reduce) has no rounding.
    rows_as_local: the planted mistake -- global_row taken as the local index."""
    x = [0.0] * n_imp
    for k, (w, g) in enumerate(zip(local_weights, global_rows)):
        x[k if rows_as_local else int(g)] = float(w)
    return x


def seam_projector(n=224):
    """A synthetic symmetric projector over n rows, in the upper storage (per row: the diagonal first if stored, then columns
    below the row, ascending), whose full rows have every length of SEAM_LENGTHS: nine hub rows spread over the list, hub h of
    length L tied to L - 1 leaf rows (the hub of 64 and the hub of 193 store no diagonal: L leaves), no hub tied to a hub; a
    leaf's length is 1 + the hubs that reach it.  Values k/8, 0 < |k| <= 8.  Returns (counts, indices, values, hubs) with
    hubs = {length: row}."""
    hubs = {L: 5 + 24 * q for q, L in enumerate(SEAM_LENGTHS)}
    hub_rows = set(hubs.values())
    leaves = [i for i in range(n) if i not in hub_rows]
    assert len(leaves) >= 193
    no_diag = {hubs[64], hubs[193]}
    pairs = {}
    for q, L in enumerate(SEAM_LENGTHS):
        h = hubs[L]
        need = L if h in no_diag else L - 1
        start = 17 * q
        for t in range(need):
            leaf = leaves[(start + t) % len(leaves)]
            pairs[(max(h, leaf), min(h, leaf))] = True

    def val(i, m):
        k = ((7 * i + 13 * m) % 17) - 8
        return (k if k else 3) / 8.0
    counts, indices, values = [], [], []
    for i in range(n):
        ent = [] if i in no_diag else [(i, val(i, i))]
        ent += [(m, val(i, m)) for m in range(i) if (i, m) in pairs]
        counts.append(len(ent))
        indices += [m + 1 for m, _ in ent]
        values += [v for _, v in ent]
    return np.array(counts, np.int64), np.array(indices, np.int64), np.array(values, np.float64), hubs


def seam_weights(n):
    """nonzero multiples of 1/4, no two neighbours alike"""
    w = []
    for i in range(n):
        k = ((5 * i) % 23) - 11
        w.append((k if k else 12) / 4.0)
    return np.array(w, np.float64)


# ------------------------------------------------------------------------------------------------ ownership and routing
PRIME = (1 << 88) + 315                                        # the FNV-128 prime
OFFSET = 0x6C62272E07BB014262B821756295C58D                    # added to det_dn before it is hashed
_M128 = 1 << 128


def owner_djb(up, dn, nranks):
    """hash = PRIME; for word in (det_up, det_dn + OFFSET): test = IEOR(word, X'5555555555555555') * PRIME;
    for j = 0, 8, ..., 120: hash = (ishft(hash, 5) + hash) + ishft(test, -j); owner = abs(mod(hash, nranks)) --
    INTEGER(16) arithmetic that wraps, shifts that are logical (the sign bit moves like any other)."""
    h = PRIME
    for word in (int(up), (int(dn) + OFFSET) % _M128):
        test = ((word ^ 0x5555555555555555) * PRIME) % _M128
        for j in range(0, 128, 8):
            h = (((h << 5) % _M128) + h + (test >> j)) % _M128
    signed = h - _M128 if h >> 127 else h
    return abs(signed) % int(nranks)                           # Fortran's mod takes the dividend's sign: |mod(x, n)| = |x| mod n


def encode(up, dn, wt, imp_distance, initiator):
    """the 32-byte wire record {up, dn, weight bits, flags} as four 64-bit words: flags & 0xFF = imp_distance (int8),
    (flags >> 8) & 0xFF = initiator (int8)"""
    bits = struct.unpack("<Q", struct.pack("<d", float(wt)))[0]
    return (int(up), int(dn), bits, (int(imp_distance) & 0xFF) | ((int(initiator) & 0xFF) << 8))


def decode(rec):
    f = int(rec[3])
    s8 = lambda b: b - 256 if b >= 128 else b
    return dict(up=int(rec[0]), dn=int(rec[1]), wt=struct.unpack("<d", struct.pack("<Q", int(rec[2])))[0],
                imp_distance=s8(f & 0xFF), initiator=s8((f >> 8) & 0xFF))


def records_to_spawns(recs):
    """an (n, 4) array of wire records as the spawn dict anneal_checker.fold takes"""
    d = [decode(r) for r in np.asarray(recs, np.uint64).reshape(-1, 4)]
    return dict(up=np.array([r["up"] for r in d], np.uint64), dn=np.array([r["dn"] for r in d], np.uint64),
                wt=np.array([r["wt"] for r in d], np.float64), imp_distance=np.array([r["imp_distance"] for r in d], np.int8),
                initiator=np.array([r["initiator"] for r in d], np.int8))


def route(records, owners, nranks, unstable=False):
    """Stable partition of the records (rows of four 64-bit words, creation order) by owner; a record of weight 0 is no walker
    and is dropped.  Returns (counts[nranks], the records of destination 0, 1, ... one after the other).
    unstable: the planted mistake -- inside a destination the order is not the creation order."""
    recs = [tuple(int(w) for w in r) for r in np.asarray(records, np.uint64).reshape(-1, 4)]
    assert len(owners) == len(recs)
    counts, out = [], []
    for q in range(int(nranks)):
        mine = [r for r, o in zip(recs, owners) if int(o) == q and decode(r)["wt"] != 0.0]
        if unstable and len(mine) > 1:
            mine = mine[1:] + mine[:1]
        counts.append(len(mine))
        out += mine
    return np.array(counts, np.int64), np.array(out, np.uint64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ comparisons
def compare_bits(what, got, want):
    """None if the two float arrays are the same bits, else the first difference as text"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return "%s: %d values, model %d" % (what, got.size, want.size)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    if len(bad):
        i = int(bad[0])
        return "%s: %d of %d differ, first at %d: %r, model %r" % (what, len(bad), got.size, i, float(got[i]), float(want[i]))
    return None


def compare_within(what, got, want, bounds):
    got, want, bounds = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bounds, np.float64)
    if got.shape != want.shape:
        return "%s: %d values, model %d" % (what, got.size, want.size)
    bad = np.nonzero(~(np.abs(got - want) <= bounds))[0]
    if len(bad):
        i = int(bad[0])
        return "%s: %d of %d outside their bound, first at %d: %r, model %r, bound %r" % (what, len(bad), got.size, i, float(got[i]), float(want[i]), float(bounds[i]))
    return None


def compare_route(send_words, send_counts, twin_records, owners, nranks):
    """the send buffer of a rank (its first sum(counts) rows) and its counts against route() of the one-rank twin's records"""
    counts, want = route(twin_records, owners, nranks)
    send_counts = np.asarray(send_counts, np.int64)
    if not np.array_equal(send_counts, counts):
        q = int(np.nonzero(send_counts != counts)[0][0])
        return "send_counts[%d] = %d, model %d" % (q, send_counts[q], counts[q])
    got = np.asarray(send_words, np.uint64).reshape(-1, 4)
    if got.shape != want.shape:
        return "%d records sent, model %d" % (len(got), len(want))
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        return "record %d of %d differs (%d do): %r, model %r" % (i, len(got), len(bad), got[i].tolist(), want[i].tolist())
    return None


def conservation(mid_step_residents, received, out):
    """out_stats[7] (nwalk_before_merge) = n0 + n_recv exactly; out_stats[14] (w_abs_before_merge) = fsum |w| over both within
    rounding_bound(n, sum).  received: (n, 4) wire records.  None, or what is wrong."""
    ws = [abs(float(w)) for w in mid_step_residents["wt"]] + [abs(decode(r)["wt"]) for r in np.asarray(received, np.uint64).reshape(-1, 4)]
    n = len(ws)
    if float(out[7]) != float(n):
        return "nwalk_before_merge = %r, %d residents + %d received = %d" % (float(out[7]), len(mid_step_residents["wt"]), n - len(mid_step_residents["wt"]), n)
    tot = math.fsum(ws)
    if not abs(float(out[14]) - tot) <= rounding_bound(n, tot):
        return "w_abs_before_merge = %r, model %r, bound %r" % (float(out[14]), tot, rounding_bound(n, tot))
    return None


def projector_against_h(args):
    """entries [k0, k1) of a projector in upper storage against -tau H_ij of proposal_checker.ChemH: (entries checked, the first
    entry outside tau * rounding_bound(terms of H_ij) or None, the largest |difference| / bound).  A plain function of plain
    arrays, so that a test can spread the entries over worker processes."""
    import proposal_checker as PC
    fcidump, orb_order, tau, rows_of, cols, values, up, dn, k0, k1 = args
    H = PC.ChemH(fcidump, [int(x) for x in orb_order])
    worst, bad = 0.0, None
    for k in range(k0, k1):
        i, m = int(rows_of[k]), int(cols[k]) - 1
        e, nt, sa = H.element(int(up[i]), int(dn[i]), int(up[m]), int(dn[m]))
        b = tau * rounding_bound(nt, sa)
        diff = abs(float(values[k]) + tau * e)
        if not diff <= b and bad is None:
            bad = (i, m, float(values[k]), -tau * e, b)
        if b:
            worst = max(worst, diff / b)
    return k1 - k0, bad, worst
