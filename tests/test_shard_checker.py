"""CPU tests of the sharded step's model (tests/shard_checker.py): the hash against the oracle's restatement of the reference,
the expansion against a dense matrix, the routing's properties, and three planted mistakes that the comparison functions of
tests/shard_phase_cases.py (the judge of the GPU cases) must report."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import shard_checker as SC


def test_owner_djb_equals_the_oracles_get_det_owner(oracle, c2_setup):
    L = oracle.lib()
    L.orc_get_det_owner.argtypes = [C.c_uint64] * 4 + [C.c_int]
    pick = np.unique(np.linspace(0, len(c2_setup.ct_up) - 1, 2000).astype(np.int64))
    assert len(pick) >= 1900
    for n in (1, 2, 3, 7, 255):
        seen = set()
        for i in pick:
            u, d = int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])
            o = SC.owner_djb(u, d, n)
            assert o == L.orc_get_det_owner(u, 0, d, 0, n), (u, d, n)
            seen.add(o)
        assert seen <= set(range(n)) and len(seen) >= min(n, 200)        # every rank is somebody's owner


def test_expand_upper_against_a_dense_symmetric_matrix():
    rs = np.random.RandomState(5)
    n = 37
    A = np.zeros((n, n))
    counts, indices, values = [], [], []
    for i in range(n):
        ent = []
        if i % 5 != 2:                       # some rows store no diagonal
            ent.append((i, float(rs.randint(-8, 9) or 1) / 8))
        for m in range(i):
            if rs.rand() < 0.3:
                ent.append((m, float(rs.randint(-8, 9) or 1) / 8))
        counts.append(len(ent))
        for m, v in ent:
            indices.append(m + 1); values.append(v)
            A[i, m] = v; A[m, i] = v
    rows = SC.expand_upper(counts, indices, values)
    B = np.zeros((n, n))
    for i, r in enumerate(rows):
        assert [c for c, _ in r] == sorted(set(c for c, _ in r))      # increasing columns, none twice
        for c, v in r:
            B[i, c] = v
    assert np.array_equal(A, B) and np.array_equal(B, B.T)
    x = rs.randint(-9, 10, n) / 4.0
    y = SC.project(rows, x, -75.75, 2.0 ** -6, exact=True)
    want = x + A @ x + (-75.75 * 2.0 ** -6) * x                       # dyadic: numpy's sums are exact here too
    assert all(SC.is_exact_double(q) for q in y) and np.array_equal(np.array([float(q) for q in y]), want)
    yf, b = SC.project(rows, x, -75.75, 2.0 ** -6, exact=False)
    assert np.array_equal(np.array(yf), want) and all(v > 0 for v in b)


def test_seam_projector_has_every_seam_length():
    counts, indices, values, hubs = SC.seam_projector()
    rows = SC.expand_upper(counts, indices, values)
    lengths = [len(r) for r in rows]
    assert set(SC.SEAM_LENGTHS) <= set(lengths)
    for L, h in hubs.items():
        assert lengths[h] == L
    assert all(v * 8 == int(v * 8) and 0 < abs(v) <= 1 for v in values)
    k = 0
    for i, c in enumerate(counts):           # the documented layout: the diagonal first, then columns below the row, ascending
        cols = [int(x) - 1 for x in indices[k:k + c]]; k += c
        below = cols[1:] if cols and cols[0] == i else cols
        assert below == sorted(below) and all(m < i for m in below)
    w = SC.seam_weights(len(counts))
    assert np.all(w != 0) and np.all(w * 4 == np.round(w * 4)) and np.all(w[1:] != w[:-1])
    x = list(w)
    for _ in range(2):                       # two steps stay exact doubles (the GPU case's precondition)
        y = SC.project(rows, x, -75.75, 2.0 ** -6, exact=True)
        y = [q * Fraction(1, 2) for q in y]
        assert all(SC.is_exact_double(q) and q != 0 for q in y)
        x = [float(q) for q in y]


def _records(n, seed):
    rs = np.random.RandomState(seed)
    recs = [SC.encode(rs.randint(1, 1 << 20), rs.randint(1, 1 << 20), (0.0 if k % 7 == 3 else (k % 11 - 5.5) / 4), (-1, 1, 2, 127)[k % 4], k % 2) for k in range(n)]
    return np.array(recs, np.uint64), rs.randint(0, 3, n)


def test_route_properties_and_the_wire_record():
    recs, owners = _records(500, 1)
    for k in (0, 1, 2, 3, 77):
        d = SC.decode(recs[k])
        assert SC.encode(d["up"], d["dn"], d["wt"], d["imp_distance"], d["initiator"]) == tuple(int(x) for x in recs[k])
    assert SC.decode(SC.encode(3, 5, -0.75, -1, 1)) == dict(up=3, dn=5, wt=-0.75, imp_distance=-1, initiator=1)
    assert SC.decode(SC.encode(3, 5, 2.0, -2, 3))["imp_distance"] == -2
    counts, out = SC.route(recs, owners, 3)
    live = [i for i in range(500) if SC.decode(recs[i])["wt"] != 0.0]
    assert counts.sum() == len(live) == len(out) and len(live) < 500           # the weight-0 records are gone
    pos = 0
    for q in range(3):
        want = [i for i in live if owners[i] == q]                              # creation order inside a destination
        assert np.array_equal(out[pos:pos + counts[q]], recs[want])
        pos += counts[q]
    c1, o1 = SC.route(recs, np.zeros(500, int), 1)
    assert np.array_equal(o1, recs[live]) and c1.tolist() == [len(live)]
    c255, _ = SC.route(recs, owners * 100, 255)
    assert (c255 == 0).sum() == 252
    assert SC.compare_route(out, counts, recs, owners, 3) is None
    sp = SC.records_to_spawns(out[:5])
    assert sp["wt"].tolist() == [SC.decode(r)["wt"] for r in out[:5]] and sp["imp_distance"].dtype == np.int8


def test_conservation():
    recs, _ = _records(60, 2)
    mid = dict(wt=np.array([0.5, -1.25, 3.0]))
    out = np.zeros(16)
    out[7] = 63
    out[14] = math.fsum([0.5, 1.25, 3.0] + [abs(SC.decode(r)["wt"]) for r in recs])
    assert SC.conservation(mid, recs, out) is None
    out[7] = 62
    assert "nwalk_before_merge" in SC.conservation(mid, recs, out)
    out[7] = 63; out[14] += 0.25
    assert "w_abs_before_merge" in SC.conservation(mid, recs, out)


# ------------------------------------------------------------------------------------------------ planted mistakes
def _seam_case():
    counts, indices, values, hubs = SC.seam_projector()
    rows = SC.expand_upper(counts, indices, values)
    return rows, SC.seam_weights(len(rows)), hubs


def test_planted_a_row_of_64_loses_its_last_term():
    rows, w, hubs = _seam_case()
    want = np.array([float(q) for q in SC.project(rows, w, -75.75, 2.0 ** -6, exact=True)])
    bad = np.array([float(q) for q in SC.project(rows, w, -75.75, 2.0 ** -6, exact=True, drop_last_at_64=True)])
    assert SC.compare_bits("weights", want, want) is None
    msg = SC.compare_bits("weights", bad, want)
    assert msg is not None and "2 of %d differ" % len(rows) in msg             # the rows of 64 and of 128, nothing else
    differ = np.nonzero(bad != want)[0].tolist()
    assert differ == sorted([hubs[64], hubs[128]])
    yf, b = SC.project(rows, w, -75.75, 2.0 ** -6, exact=False)
    assert SC.compare_within("weights", bad, yf, b) is not None and SC.compare_within("weights", want, yf, b) is None


def test_planted_global_row_taken_as_the_local_index():
    rows, w, hubs = _seam_case()
    n = len(rows)
    mine = [g for g in range(n) if g % 3 == 1]                                 # a rank that owns every third row
    x_good = SC.gather(w[mine], mine, n)
    x_bad = SC.gather(w[mine], mine, n, rows_as_local=True)
    assert SC.compare_bits("x_global", x_good, x_good) is None
    assert SC.compare_bits("x_global", x_bad, x_good) is not None
    assert [x_good[g] for g in mine] == w[mine].tolist() and sum(1 for v in x_good if v != 0) == len(mine)
    # the sum over three such ranks is the whole vector, exactly
    tot = np.zeros(n)
    for r in range(3):
        own = [g for g in range(n) if g % 3 == r]
        tot += np.array(SC.gather(w[own], own, n))
    assert np.array_equal(tot, w)
    # and the projection of the owned rows through the wrong map differs from the model in its bits
    good = [float(q) for q in SC.project(rows, tot, -75.75, 2.0 ** -6, exact=True, only=mine)]
    wrong = [float(q) for q in SC.project(rows, tot, -75.75, 2.0 ** -6, exact=True, only=range(len(mine)))]
    assert SC.compare_bits("weights", wrong, good) is not None


def test_planted_routing_that_is_not_stable():
    recs, owners = _records(500, 3)
    counts, good = SC.route(recs, owners, 3)
    c_bad, bad = SC.route(recs, owners, 3, unstable=True)
    assert np.array_equal(counts, c_bad) and sorted(map(tuple, good.tolist())) == sorted(map(tuple, bad.tolist()))      # the same records, the same counts
    assert SC.compare_route(good, counts, recs, owners, 3) is None
    msg = SC.compare_route(bad, c_bad, recs, owners, 3)
    assert msg is not None and "differs" in msg
    assert "send_counts" in SC.compare_route(good, counts + np.array([1, -1, 0]), recs, owners, 3)
