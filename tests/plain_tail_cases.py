"""Directed inputs for the tail of a step with semistochastic = f -- k_merge, the joins of join_walker2 (k_join_gather + k_join_par
in the COUNTER discipline, the one-lane k_join in REPLAY or under SQMC_SERIAL_JOIN), the plain branch of k_round, k_compact --
their expected output from the independent model (anneal_checker.plain_step), and the program that puts them through
sqmc_gpu_annihilate.  The pattern is anneal_edge_cases.py's:

  solve(cases, ...), write(path, ...)    in the test process: folds and joins every case with the model -- once with the draws of
                        the COUNTER discipline, once with REPLAY's -- and writes everything a child needs to one file;
  python plain_tail_cases.py FILE VARIANT    in a fresh child whose environment selects the variant: every case through the
                        library, the tail asserted (radix, no spawn-only merge), walkers bit for bit, sums within their bounds,
                        and the draw-free chain layer (anneal_checker.chain_layer).  One JSON line per case; exit 0: all equal,
                        1: a mismatch, 3: a HIP failure (it stops at once and starts nothing more on the GPU).

Sets: A -- anneal_edge_cases.build_cases for the 256-slot tile of k_merge, weights multiples of 0.25 with min_wt 0.25: join-free;
B -- join cases, min_wt 0.5, weights multiples of Q = 2^-13, r_initiator = -1 (nothing is reset or demoted, so the slot of every
candidate is the slot it was written on); C -- who carries a chain's weight, judged by its binomial bounds; D -- one list of more
than JP_CW x JP_TILE slots, for the reload of k_join_par's window of chunk counts.

The tile and chunk sizes are read from walk_kernels.h, so a changed constant moves the cases with it.
"""
import json
import math
import os
import pickle
import re
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import anneal_edge_cases as EC          # noqa: E402

SEED = EC.SEED
MWALK = 40960
Q = 2.0 ** -13                        # the weight quantum of sets B-D
MIN_WT = 0.5
UNITS = int(MIN_WT / Q)               # min_wt in quanta: 4096

# variant -> (environment, rng_mode)
VARIANTS = {
    "plain_counter": ({}, 1),
    "plain_counter_serial_join": ({"SQMC_SERIAL_JOIN": "1"}, 1),
    "plain_replay": ({}, 0),
    "plain_unpacked": ({"SQMC_FORCE_UNPACKED": "1"}, 1),
}
C_VARIANTS = ("plain_counter", "plain_counter_serial_join")


def kernel_constants():
    """TPB, JOIN_TILE, JP_TILE, JP_CW as the kernels are compiled with them"""
    csrc = os.path.join(ROOT, "sqmc_amd", "csrc")
    txt = open(os.path.join(csrc, "walk_kernels.h")).read()
    g = lambda name, t: int(re.search(r"#define %s (\d+)" % name, t).group(1))
    return dict(TPB=g("TPB", open(os.path.join(csrc, "sqmc_gpu.hip")).read()), JOIN_TILE=g("JOIN_TILE", txt), JP_TILE=g("JP_TILE", txt), JP_CW=g("JP_CW", txt))


def generated_universe(norb, nup, ndn, n_dn=3):
    """a sorted universe of determinants that owes nothing to C(T): every nup-of-norb up string with n_dn fixed dn strings"""
    from itertools import combinations
    ups = sorted(sum(1 << o for o in c) for c in combinations(range(norb), nup))
    dns = sorted({(1 << ndn) - 1, (1 << ndn) | ((1 << (ndn - 1)) - 1), sum(1 << (2 * k) for k in range(ndn))})[:n_dn]
    assert all(bin(d).count("1") == ndn for d in dns) and all(bin(u).count("1") == nup for u in ups[:50])
    uu = np.repeat(np.array(ups, np.uint64), len(dns))
    ud = np.tile(np.array(dns, np.uint64), len(ups))
    return uu, ud


def rannyu48(state):
    """rannyu (rannyu.f90:54-74) on the 48-bit integer its four 12-bit limbs spell: x <- 11^13 x mod 2^48, the real is x 2^-48.
    Returns (new state, real)."""
    state = (state * 34522712143931) & 0xFFFFFFFFFFFF
    return state, state * 2.0 ** -48


def rannyu_seed(seed):
    """setrn: the last limb made odd"""
    l = [int(x) for x in seed]
    l[3] = 2 * (l[3] // 2) + 1
    return ((l[0] << 36) + (l[1] << 24) + (l[2] << 12) + l[3]) & 0xFFFFFFFFFFFF


def rannyu_limbs(state):
    return [(state >> 36) & 4095, (state >> 24) & 4095, (state >> 12) & 4095, state & 4095]


class ReplayDraws:
    """REPLAY: the draws are the rannyu stream in join order, whatever the index"""

    def __init__(self, seed=SEED):
        self.x, self.n = rannyu_seed(seed), 0

    def __call__(self, i):
        self.x, r = rannyu48(self.x)
        self.n += 1
        return r


def jp_tiles(counts, consts):
    """k_join_par's greedy packing restated: chunks are appended while the tile's candidates stay <= JP_TILE, never across a
    window of JP_CW chunks.  counts: candidates of one sign per chunk.  Returns [(first chunk, chunk behind the last, candidates)]."""
    tiles, ci, wbase, n = [], 0, -consts["JP_CW"], len(counts)
    while ci < n:
        if ci >= wbase + consts["JP_CW"]:
            wbase = ci
        cj, nc = ci, 0
        while cj < n and cj < wbase + consts["JP_CW"] and nc + counts[cj] <= consts["JP_TILE"]:
            nc += counts[cj]; cj += 1
        assert cj > ci, "a chunk alone always fits"
        tiles.append((ci, cj, nc)); ci = cj
    return tiles


def layout(case, heads, consts):
    """where the kernels meet every candidate.  heads: the merged list (model).  Returns dict(slot: sorted-list slot per head,
    cand[sign]: head indices of the candidates in list order, tiles[sign]: jp_tiles, at[sign]: (tile, slot in the tile, 1-based)
    per candidate, nall)."""
    shift = np.uint64(32)
    key = lambda d: (d["up"].astype(np.uint64) << shift) | d["dn"].astype(np.uint64)
    assert not (case["sp"]["wt"] == 0).any(), "a zero-weight spawn takes a slot at the end of the sorted list: sets B-D have none"
    allk = np.sort(np.concatenate([key(case["res"]), key(case["sp"])]))
    slot = np.searchsorted(allk, key(heads), side="left")
    nall = len(allk)
    nchunks = (nall + consts["JP_TILE"] - 1) // consts["JP_TILE"]
    w, ini = heads["wt"], heads["initiator"]
    out = dict(slot=slot, nall=nall, cand={}, tiles={}, at={})
    for sign in (1, -1):
        idx = np.nonzero((w * sign > 0) & (np.abs(w) < case["prm"]["min_wt"]) & (ini < 3))[0]
        chunk = slot[idx] // consts["JP_TILE"]
        counts = np.bincount(chunk, minlength=nchunks).tolist() if len(idx) else [0] * nchunks
        tiles = jp_tiles(counts, consts)
        first = np.zeros(nchunks + 1, np.int64)          # per chunk: (its tile, candidates of the tile in front of it)
        tile_of = np.zeros(nchunks + 1, np.int64)
        for t, (a, b, nc) in enumerate(tiles):
            run = 0
            for c in range(a, b):
                tile_of[c], first[c] = t, run
                run += counts[c]
        at, seen = [], {}
        for i, c in zip(idx.tolist(), chunk.tolist()):
            k = seen.get(c, 0); seen[c] = k + 1
            at.append((int(tile_of[c]), int(first[c]) + k + 1))
        out["cand"][sign], out["tiles"][sign], out["at"][sign] = idx, tiles, at
    return out


def chains_by_ordinal(lay, chains):
    """the model's chains with every member named by its ordinal among its sign's candidates: {sign: [(first, last, closed, total)]}"""
    out = {}
    for sign in (1, -1):
        ordinal = {int(h): k for k, h in enumerate(lay["cand"][sign])}
        out[sign] = [(ordinal[m[0]], ordinal[m[-1]], closed, total) for m, total, closed in chains[sign]]
        for m, _, _ in chains[sign]:
            assert [ordinal[x] for x in m] == list(range(ordinal[m[0]], ordinal[m[0]] + len(m))), "a chain is a stretch of consecutive candidates"
    return out


# ------------------------------------------------------------------------------------------------ building the join cases
class PB(EC.Builder):
    """anneal_edge_cases.Builder with its traffic scaled to non-candidates (multiples of min_wt) and lone candidates of k quanta"""

    def __init__(self, uu, ud, seed):
        super().__init__(uu, ud, seed)
        self.n_cand = {1: 0, -1: 0}
        self.flip = 0

    def _w(self, nonzero=False):
        while True:
            w = int(self.rs.randint(-8, 9)) / 2.0
            if w != 0 or not nonzero:
                return w

    def cand(self, units, sign, how=None):
        """one lone candidate of `units` quanta, a resident or a spawn on a determinant of its own; returns its ordinal among its sign's"""
        assert 0 < units < UNITS
        self.flip += 1
        how = self.flip % 3 if how is None else how
        if how == 0:
            self.resident(sign * units * Q, int(self.rs.choice([1, 2, 4])), 1 + self.flip % 2)
        else:
            self.spawn(self.fresh(), sign * units * Q, int(self.rs.choice([1, 2, 5])), self.flip % 2)
        self.n_cand[sign] += 1
        return self.n_cand[sign] - 1

    def other(self, kind=None):
        """one lone walker the joins must not touch"""
        kind = int(self.rs.randint(0, 7)) if kind is None else kind
        s = 1.0 if self.rs.rand() < 0.5 else -1.0
        if kind == 0:
            self.resident(s * MIN_WT, 2, 1)                      # |w| == min_wt: no candidate (the test is strict)
        elif kind == 1:
            self.resident(s * 1024 * Q, 1, 3, int(s))            # a small permanent initiator (r_initiator -1: its weight is not reset)
        elif kind == 2:
            self.resident(0.0, 0, 2)                             # a zero-weight head of the deterministic space: dropped, by 7075
        elif kind == 3:
            self.resident(0.0, -2, 1)
        elif kind == 4:
            self.spawn(self.fresh(), s * MIN_WT, 2, 1)
        elif kind == 5:
            self.spawn(self.fresh(), s * (MIN_WT + Q), 3, 0)     # one quantum above min_wt
        else:
            self.resident(s * 1.5, 3, 2)

    def lay(self, cands, upto, kinds=None):
        """the candidates [(units, sign)] in their order on the slots up to `upto`, lone untouchables everywhere between them"""
        n_other = upto - self.slots() - len(cands)
        assert n_other >= 0, (upto, self.slots(), len(cands))
        total = len(cands) + n_other
        pos = set(self.rs.choice(total, len(cands), replace=False).tolist()) if total else set()
        it = iter(cands)
        for k in range(total):
            if k in pos:
                self.cand(*next(it))
            else:
                self.other(None if kinds is None else kinds[int(self.rs.randint(0, len(kinds)))])
        assert self.slots() == upto

    def closed(self, L):
        """L weights whose running sum first exceeds min_wt on the last one"""
        assert 2 <= L < UNITS
        a = UNITS // L
        return [a] * (L - 1) + [UNITS + 1 - a * (L - 1)]

    def closed_chains(self, n, sign):
        """n candidates of one sign that fall into closed chains of 2 to 9 members"""
        assert n >= 2
        out = []
        while n:
            L = min(n, int(self.rs.randint(2, 10)))
            if n - L == 1:
                L = n
            out += [(u, sign) for u in self.closed(L)]
            n -= L
        return out

    def weave(self, a, b):
        """two sequences in one, each in its own order"""
        take = np.zeros(len(a) + len(b), bool)
        take[self.rs.choice(len(a) + len(b), len(a), replace=False)] = True
        ia, ib = iter(a), iter(b)
        return [next(ia) if t else next(ib) for t in take]

    def done(self, name, **meta):
        self.filler(int(self.rs.randint(20, 60)))
        rfi = 0.5 if len(name) % 2 else 1.0
        return self.finish(name, prm=dict(semistochastic=0, min_wt=MIN_WT, always_spawn_cutoff_wt=MIN_WT, r_initiator=-1.0, reweight_factor_inv=rfi), **meta)


def build_join_cases(uu, ud, consts):
    """set B.  meta['pos']: [(sign, ordinal, tile, slot)] a candidate must sit on; meta['chain']: [(sign, first, last, closed)] chains
    that must be among the model's (ordinals among the sign's candidates); the CPU test asserts both."""
    C, JT = consts["JP_TILE"], consts["JOIN_TILE"]
    cases, seed = [], [7000]

    def B():
        seed[0] += 1
        return PB(uu, ud, seed[0])

    def done_nofill(b, name, **meta):
        return b.finish(name, prm=dict(semistochastic=0, min_wt=MIN_WT, always_spawn_cutoff_wt=MIN_WT, r_initiator=-1.0, reweight_factor_inv=0.5 if len(name) % 2 else 1.0), **meta)

    n0 = (3 * C) // 4 - 36
    n1 = C - n0 + 52                      # 1500 and 600 at C = 2048: together they do not fit one tile
    assert n0 + n1 > C and n0 > 600 and n1 > 400
    for sign, tag in ((1, "pos"), (-1, "neg")):
        # a chain closes on the last candidate of a tile, the next chain begins on the first candidate of the next tile
        b = B()
        b.lay(b.weave(b.closed_chains(n0, sign), b.closed_chains(200, -sign)), C)
        b.lay(b.weave(b.closed_chains(n1, sign), b.closed_chains(77, -sign)), 2 * C)
        cases.append(b.done("chain_closes_on_a_tiles_last_candidate_" + tag, pos=[(sign, n0 - 1, 0, n0), (sign, n0, 1, 1)], chain=[(sign, None, n0 - 1, True), (sign, n0, None, True)]))
        # a chain left open by a tile and closed in the next
        b = B()
        b.lay(b.closed_chains(n0 - 3, sign) + [(100, sign)] * 3, C)
        b.lay([(100, sign), (UNITS - 96, sign)] + b.closed_chains(n1 - 2, sign), 2 * C)
        cases.append(b.done("chain_open_across_a_tile_" + tag, pos=[(sign, n0 - 1, 0, n0), (sign, n0 + 1, 1, 2)], chain=[(sign, n0 - 3, n0 + 1, True)]))
        # a tile takes over an open chain, and its own last chain closes on its last candidate: the open flag must fall again (a kernel
        # that never clears it joins the next tile's first candidate to a chain that is closed -- tried once: only this case and C notice)
        b = B()
        b.lay(b.closed_chains(n0 - 3, sign) + [(100, sign)] * 3, C)
        b.lay([(100, sign), (UNITS - 96, sign)] + b.closed_chains(n0 - 2, sign), 2 * C)
        b.lay(b.closed_chains(n1, sign), 3 * C)
        cases.append(b.done("open_chain_taken_over_then_closed_on_the_tiles_last_candidate_" + tag, mwalk=4 * C,
                            pos=[(sign, n0, 1, 1), (sign, 2 * n0 - 1, 1, n0), (sign, 2 * n0, 2, 1)],
                            chain=[(sign, n0 - 3, n0 + 1, True), (sign, None, 2 * n0 - 1, True), (sign, 2 * n0, None, True)]))
        # ... and open across three tiles: the middle tile is full (nc == JP_TILE) and lies inside the chain altogether
        b = B()
        b.lay(b.closed_chains(n0 - 500, sign) + [(1, sign)] * 500, C)
        b.lay([(1, sign)] * C, 2 * C)
        b.lay([(1, sign)] * 10 + [(UNITS - 96, sign)] + b.closed_chains(n1 - 11, sign), 3 * C)
        cases.append(b.done("chain_open_across_three_tiles_" + tag, mwalk=4 * C, pos=[(sign, n0 - 1, 0, n0), (sign, n0, 1, 1), (sign, n0 + C - 1, 1, C), (sign, n0 + C, 2, 1)],
                            chain=[(sign, n0 - 500, n0 + C + 10, True)]))
        # one chunk of JP_TILE lone candidates of one quantum: the tile is exactly full and its chain still open at its end
        b = B()
        b.lay([(1, sign)] * C, C)
        b.lay([(1, sign)] * 100 + [(UNITS - C - 50, sign)] + b.closed_chains(300, sign), 2 * C)
        cases.append(b.done("full_tile_of_single_quanta_" + tag, pos=[(sign, 0, 0, 1), (sign, C - 1, 0, C), (sign, C, 1, 1)], chain=[(sign, 0, C + 100, True)]))
        # the rest of the list has no candidate of the sign: the chain stays open (at this packing the empty chunks join its tile;
        # the tile with no candidate behind an open chain is case D's)
        b = B()
        b.lay(b.weave(b.closed_chains(300, sign) + [(100, sign)] * 3, b.closed_chains(150, -sign)), C)
        b.lay(b.closed_chains(500, -sign), 3 * C)
        cases.append(b.done("chain_left_open_no_candidate_behind_" + tag, mwalk=4 * C, chain=[(sign, 300, 302, False)]))
    # chunks of C/2 + C/2 candidates: one tile, exactly full, a chain across the chunk seam; C/2 + 1 and C/2: two tiles
    for extra in (0, 1):
        b = B()
        h = C // 2
        first = b.closed_chains(h - 2 + extra, 1) + [(100, 1)] * 2
        b.lay(b.weave(first, b.closed_chains(300, -1)), C)
        b.lay(b.weave([(100, 1), (UNITS - 96, 1)] + b.closed_chains(h - 2, 1), b.closed_chains(200, -1)), 2 * C)
        k = h + extra
        cases.append(b.done("chunks_of_%d_and_%d_candidates" % (k, h), pos=[(1, k - 1, 0, k), (1, k, 0, k + 1) if not extra else (1, k, 1, 1), (1, k + h - 1, extra, C if not extra else h)],
                            chain=[(1, k - 2, k + 1, True)], tiles={1: 1 + extra}))
    # a running sum exactly min_wt does not close (the test is strict); the next quantum does
    b = B()
    b.lay(b.closed_chains(40, 1) + [(UNITS // 2, 1), (UNITS // 2, 1), (1, 1)] + b.closed_chains(40, 1), 700)
    b.lay(b.closed_chains(30, -1) + [(UNITS // 2, -1), (UNITS // 2, -1), (1, -1)] + b.closed_chains(31, -1), 1200)
    cases.append(b.done("sum_equal_min_wt_inside_a_tile", chain=[(1, 40, 42, True), (-1, 30, 32, True)]))
    b = B()
    b.lay(b.closed_chains(n0 - 2, 1) + [(UNITS // 2, 1), (UNITS // 2, 1)], C)
    b.lay([(1, 1)] + b.closed_chains(n1 - 1, 1), 2 * C)
    cases.append(b.done("sum_equal_min_wt_on_a_tiles_last_candidate", pos=[(1, n0 - 1, 0, n0), (1, n0, 1, 1)], chain=[(1, n0 - 2, n0, True)]))
    # walkers that must not be touched, one of every kind between the members of one chain
    b = B()
    b.filler(300)
    for kind in (0, 1, 2, 3):
        b.cand(500, 1); b.other(kind)
    b.cand(500, 1); b.cand(300, -1); b.cand(500, 1); b.other(1); b.cand(UNITS - 299, -1); b.cand(UNITS - 500, 1)
    cases.append(b.done("untouched_walkers_between_the_members_of_a_chain", chain=[(1, 0, 6, True), (-1, 0, 1, True)]))
    # positive and negative candidates strictly alternating over more than one chunk
    b = B()
    p, n = b.closed_chains(C // 2 + 300, 1), b.closed_chains(C // 2 + 300, -1)
    for x, y in zip(p, n):
        b.cand(*x); b.cand(*y)
    cases.append(b.done("signs_alternate_over_two_chunks"))
    # the list's length against the chunk: candidates of both signs at both ends of the last chunk
    for nall in (C - 1, C, C + 1, 2 * C, 2 * C + 1):
        b = B()
        last = ((nall - 1) // C) * C
        if last:
            b.lay(b.weave(b.closed_chains(400, 1)[:-1], b.closed_chains(300, -1)[:-1]), last)          # both chains still open at the seam
        ln = nall - last
        ends = [(700, 1), (900, -1)]
        if ln >= 8:
            for x in ends:
                b.cand(*x)
            b.lay(b.weave(b.closed_chains(50, 1), b.closed_chains(50, -1)), nall - 2)
            for x in ends[::-1]:
                b.cand(*x)
        else:
            b.cand(*ends[nall % 2])
        assert b.slots() == nall
        cases.append(done_nofill(b, "nall_%d" % nall, nall=nall, mwalk=3 * C))
    b = B()
    b.lay(b.weave(b.closed_chains(300, 1), b.closed_chains(300, -1)), C)
    for x in b.weave(b.closed_chains(400, 1)[:-1], b.closed_chains(300, -1)):
        b.cand(*x)
    cases.append(done_nofill(b, "every_slot_of_the_partial_last_chunk_a_candidate", nall=C + 699, mwalk=3 * C))
    # degenerate lists
    b = B(); b.lay([], 900)
    cases.append(b.done("no_candidate", joins=0))
    b = B(); b.lay([(77, -1)], 900)
    cases.append(b.done("a_single_candidate", joins=0, chain=[(-1, 0, 0, False)]))
    b = B(); b.lay([(100, 1)] * 40 + [(96, 1)], 900)
    cases.append(b.done("all_candidates_in_one_open_chain_of_exactly_min_wt", joins=40, chain=[(1, 0, 40, False)]))
    b = B(); b.lay(b.closed_chains(500, -1), 1500, kinds=(0, 2, 3, 6))
    cases.append(b.done("candidates_of_one_sign_only"))
    # candidates that come out of the fold
    b = B()
    T = consts["TPB"]
    b.lay(b.closed_chains(60, 1)[:-1], T - 5)
    u = b.fresh()
    for w in [306, -300] + [200, -200] * 4:                    # slots T-5 .. T+4: +6 quanta in all, across the seam of k_merge's tile
        b.spawn(u, w * Q, 2, 1)
    b.lay(b.closed_chains(30, 1), T + 200)
    r = b.resident(1.0, 2, 2)                                  # a resident brought below min_wt by spawns of the other sign
    for w in (-0.5, -0.25, -0.125):
        b.spawn(r, w, 2, 1)
    b.lay(b.closed_chains(20, 1), T + 300)
    u = b.fresh()                                              # a run that sums to exactly 0: discarded, no candidate
    for w in (0.25, -0.125, -0.125):
        b.spawn(u, w, 2, 1)
    b.lay(b.closed_chains(20, 1) + b.closed_chains(9, -1), T + 400)
    cases.append(b.done("candidates_that_come_out_of_the_fold", fold_seam=T - 5))
    # the one-lane k_join stages the list in tiles of JOIN_TILE slots
    b = B()
    b.lay(b.weave(b.closed_chains(100, 1), [(1, -1)]), JT - 2)
    b.cand(100, 1, how=0); b.cand(100, 1, how=1); b.cand(100, 1, how=1); b.cand(UNITS - 200, 1, how=0)          # slots JOIN_TILE-2 .. JOIN_TILE+1
    b.lay([(2, -1)], 2 * JT - 10, kinds=(0, 1, 6))             # the negative chain: one member in each of three staging tiles
    b.lay([], 2 * JT + 5, kinds=(0, 2, 6))
    b.lay([(UNITS - 2, -1)] + b.closed_chains(10, -1), 2 * JT + 300)
    cases.append(b.done("chains_across_the_staging_tiles_of_the_serial_join", chain=[(1, 100, 103, True), (-1, 0, 2, True)], join_seam=JT))
    return cases


# ------------------------------------------------------------------------------------------------ C: who carries the weight
CARRY = (1, 2, 3, 3)          # sixteenths: the running sums 1/16, 3/16, 6/16, 9/16 -- every chain closes on its fourth member


def carrier_case(uu, ud, n_chains=4096):
    """n_chains aligned positive chains of (1, 2, 3, 3)/16 and as many negative ones, lone walkers on determinants of their own.
    Member q carries the chain's weight with probability a_q / 9 (the reference's rule: P(q) = (a_q / t_q) prod_{k > q} t_{k-1} / t_k
    = a_q / t_m, t the running sums)."""
    b = PB(uu, ud, 9100)
    members = {1: [], -1: []}
    for c in range(n_chains):
        for sign in (1, -1):
            at = []
            for a in CARRY:
                b.cand(a * UNITS // 8, sign, how=(c + len(at)) % 3)
                at.append(b.next - 1)
            members[sign].append(at)
            if c % 7 == 0:
                b.other()
    case = b.finish("carrier_of_%d_chains_per_sign" % n_chains, prm=dict(semistochastic=0, min_wt=MIN_WT, always_spawn_cutoff_wt=MIN_WT, r_initiator=-1.0, reweight_factor_inv=1.0),
                    kind="carrier", only=C_VARIANTS, mwalk=b.slots() + 64)
    case["members"] = {s: (uu[np.array(v, np.int64)], ud[np.array(v, np.int64)]) for s, v in members.items()}          # (up, dn) per chain and class
    return case


def carrier_verdict(case, up, dn, wt):
    """every chain has exactly one survivor, of weight sign x 9/16, and the carriers per class lie within 5 binomial standard
    deviations of n a_q / 9.  Returns (None or what is wrong, {sign: counts per class})."""
    have = {(int(u), int(d)): float(w) for u, d, w in zip(up, dn, wt)}
    counts = {}
    for sign in (1, -1):
        cnt = [0, 0, 0, 0]
        for mu, md in zip(case["members"][sign][0].tolist(), case["members"][sign][1].tolist()):
            alive = [q for q in range(4) if (mu[q], md[q]) in have]
            if len(alive) != 1 or have[(mu[alive[0]], md[alive[0]])] != sign * 9.0 / 16.0:
                return "a chain with survivors %r" % (alive,), None
            cnt[alive[0]] += 1
        counts[sign] = cnt
    n = len(case["members"][1][0])
    for sign in (1, -1):
        for q, a in enumerate(CARRY):
            pr = a / 9.0
            if abs(counts[sign][q] - n * pr) > 5.0 * math.sqrt(n * pr * (1 - pr)):
                return "sign %+d class %d: %d carriers, binomial mean %.1f, sigma %.1f" % (sign, q, counts[sign][q], n * pr, math.sqrt(n * pr * (1 - pr))), counts
    return None, counts


def carrier_bounds(n=4096):
    return [(n * a / 9.0 - 5.0 * math.sqrt(n * a / 9.0 * (1 - a / 9.0)), n * a / 9.0 + 5.0 * math.sqrt(n * a / 9.0 * (1 - a / 9.0))) for a in CARRY]


# ------------------------------------------------------------------------------------------------ D: the window of chunk counts
def window_case(uu, ud, consts, run_len=525):
    """One list of a little more than JP_CW x JP_TILE sorted slots, almost all of it long one-sign runs of dyadic spawns.  Lone
    candidates: a positive chain open across the boundary between chunk JP_CW - 1 and chunk JP_CW, closed behind it, and further
    positive chains behind that; a negative chain open at the boundary with no negative candidate behind it -- the second window's
    tile has no candidate and an open chain.  No candidate in the partial last chunk.  run_len: the thinned copy takes 5."""
    C, W = consts["JP_TILE"], consts["JP_CW"]
    Bd = C * W
    nall = Bd + 2 * C + 300
    rs = np.random.RandomState(31337)
    pb = PB(uu, ud, 1)          # for closed_chains only
    pb.rs = rs
    at = {}

    def place(cands, lo, hi, fixed=None):
        free = np.setdiff1d(np.arange(lo, hi), np.array(sorted(at), np.int64))
        slots = np.sort(rs.choice(free, len(cands), replace=False))
        for s, c in zip(slots.tolist(), cands):
            at[s] = c
    place(pb.weave(pb.closed_chains(200, 1), pb.closed_chains(150, -1)), 10, 2 * C - 50)
    place(pb.weave(pb.closed_chains(100, 1), pb.closed_chains(100, -1)), (W // 2) * C - 900, (W // 2) * C + 2100)
    at[Bd - 1] = (100, 1)                                                       # the open positive chain ends on the window's last slot
    place(pb.weave(pb.closed_chains(40, 1) + [(100, 1)] * 2, pb.closed_chains(30, -1) + [(100, -1)] * 2), Bd - C + 5, Bd - 1)
    at[Bd] = (100, 1)                                                           # ... and goes on on the next window's first
    place([(UNITS - 300, 1)] + pb.closed_chains(120, 1), Bd + 1, Bd + 2 * C)
    n_pos = sum(1 for v in at.values() if v[1] > 0)
    run_det, run_n, run_w, run_res = [], [], [], []
    c_det, c_w, c_res = [], [], []
    det, s = 8, 0
    for c in sorted(at) + [nall]:
        gap = c - s if run_len >= 64 else min(c - s, 40)
        while gap > 0:
            L = min(gap, run_len if run_len >= 64 else int(rs.randint(1, run_len + 1)))
            run_det.append(det); run_n.append(L); run_w.append(float(rs.choice([0.5, 0.75, 1.0, 2.0])) * (1 if rs.rand() < 0.55 else -1)); run_res.append(bool(rs.rand() < 0.5))
            det += 1; gap -= L
        if c < nall:
            c_det.append(det); c_w.append(at[c][0] * Q * at[c][1]); c_res.append(len(c_det) % 3 == 0); det += 1
        s = c + 1
    if run_len < 64:          # the thinned copy: the same candidates between short runs
        nall = sum(run_n) + len(c_det)
    assert det < len(uu)
    run_res[0] = True          # the list's first record: a resident of the deterministic space (the door wants one)
    run_det, run_n, run_w, run_res = np.array(run_det), np.array(run_n), np.array(run_w), np.array(run_res)
    c_det, c_w, c_res = np.array(c_det), np.array(c_w), np.array(c_res)
    r_det = np.concatenate([run_det[run_res], c_det[c_res]]); r_w = np.concatenate([run_w[run_res], c_w[c_res]])
    o = np.argsort(r_det)
    r_det, r_w = r_det[o], r_w[o]
    nsp = run_n - run_res
    s_det = np.concatenate([np.repeat(run_det, nsp), c_det[~c_res]]); s_w = np.concatenate([np.repeat(run_w, nsp), c_w[~c_res]])
    o = rs.permutation(len(s_det))
    s_det, s_w = s_det[o], s_w[o]
    from anneal_checker import default_params
    case = dict(name="window_of_chunk_counts_reloaded" if run_len >= 64 else "window_case_thinned",
                prm=default_params(semistochastic=0, min_wt=MIN_WT, always_spawn_cutoff_wt=MIN_WT, r_initiator=-1.0, reweight_factor_inv=0.5),
                meta=dict(kind="window", mwalk=max(nall + 4096, 2300000 if run_len >= 64 else 0), nall=nall, n_pos=n_pos, boundary=Bd),
                res=dict(up=uu[r_det], dn=ud[r_det], wt=r_w, imp_distance=np.full(len(r_det), 2, np.int8), initiator=np.full(len(r_det), 2, np.int8), perm_sign=np.zeros(len(r_det), np.int8)),
                sp=dict(up=uu[s_det], dn=ud[s_det], wt=s_w, imp_distance=rs.choice([1, 2, 3], len(s_det)).astype(np.int8), initiator=rs.randint(0, 2, len(s_det)).astype(np.int8)))
    assert len(case["res"]["up"]) + len(case["sp"]["up"]) == nall and r_det[0] == 8
    case["res"]["imp_distance"][0] = 0
    return case


def is_exact(case):
    """every weight a multiple of Q, and the sum of all of them far below 2^53 quanta: any order of additions gives the same doubles"""
    w = np.concatenate([case["res"]["wt"], case["sp"]["wt"]]) / Q
    return bool(np.all(w == np.floor(w)) and np.abs(w).sum() < 2.0 ** 50)


# ------------------------------------------------------------------------------------------------ the model's answers
def set_a(uu, ud):
    """anneal_edge_cases.build_cases at k_merge's own tile, as plain steps"""
    consts = kernel_constants()
    cases = EC.build_cases(uu, ud, consts["TPB"], EC.bucket_constants())
    for c in cases:
        c["prm"] = dict(c["prm"], semistochastic=0)
        c["meta"]["set"] = "A"
    return cases


def answer(case, ct, counter_draw, exact=True):
    """the model's output for both disciplines, its sums and their bounds, heads and chains for the draw-free layer"""
    import anneal_checker as AC
    want = {}
    for mode in ((1,) if case["meta"].get("kind") in ("window", "carrier") else (1, 0)):
        draws = ReplayDraws() if mode == 0 else counter_draw
        m = AC.plain_step(case["res"], case["sp"], case["prm"], draws, exact=exact)
        st, spread = AC.sums(m, case["prm"], ct, m["n_before"], m["w_abs_before"])
        want[mode] = dict({k: m[k] for k in ("up", "dn", "wt", "imp_distance", "initiator")}, stats=st, joins=m["joins"],
                          rng=rannyu_limbs(draws.x) if mode == 0 else None,
                          stat_bound={k: 4.0 * spread[k][0] * 2.0 ** -53 * spread[k][1] for k in spread})          # proposal_checker.rounding_bound of this list's own terms
        # w2_gen is exact in any order of additions only while the squares, in units of the square of the weights' own quantum, sum to
        # less than 2^53; case D's do not (weights of hundreds at a quantum of 2^-14: 57 bits), and get the bound of a sum of n terms
        ws = [Fraction(x) for x in m["wt"].tolist()]
        den = max([w.denominator for w in ws] + [1])
        s2 = sum(w * w for w in ws)
        if not s2 * den * den < 2 ** 53:
            want[mode]["stat_bound"][8] = 4.0 * len(ws) * 2.0 ** -53 * float(s2)
        if m["joins"] == 0:
            want[0] = dict(want[1], rng=rannyu_limbs(rannyu_seed(SEED)))
            break
    case["want"] = want
    case["heads"], case["chains"] = m["heads"], m["chains"]
    case["n_discarded"] = len(m["discarded"])
    return m


def solve(cases, ct, counter_draw):
    """the model's answer to every case, with the assertions that make a case what it claims to be"""
    import anneal_checker as AC
    for c in cases:
        if c["meta"].get("set") == "A":
            AC.check_precondition(c["res"], c["sp"], c["prm"])          # exact, and join-free: no head below min_wt
        else:
            assert is_exact(c), c["name"]
        m = answer(c, ct, counter_draw, exact=c["meta"].get("kind") != "window")
        assert (m["joins"] == 0) if c["meta"].get("set") == "A" else True
        for mode in sorted(c["want"]):
            bad = AC.chain_layer(c["heads"], c["chains"], c["prm"], c["want"][mode])
            assert not bad, (c["name"], mode, bad[:3])
    return cases


def write(path, tables, cases, ct):
    """the file a child reads"""
    keys = sorted(ct)
    blob = dict(tables=tables, cases=cases, consts=kernel_constants(),
                ct=dict(up=np.array([k[0] for k in keys], np.uint64), dn=np.array([k[1] for k in keys], np.uint64),
                        num=np.array([ct[k][0] for k in keys]), den=np.array([ct[k][1] for k in keys])))
    with open(path, "wb") as f:
        pickle.dump(blob, f, protocol=4)
    return cases


# ------------------------------------------------------------------------------------------------ the child
def run_case(blob, variant, case):
    import anneal_checker as AC
    import sqmc_amd
    env, rng_mode = VARIANTS[variant]
    res, sp, prm, meta = case["res"], case["sp"], case["prm"], case["meta"]
    want = case["want"][rng_mode]
    t0 = time.time()
    g = EC._ctx(blob, rng_mode, meta.get("mwalk", MWALK), int((res["imp_distance"] == 0).sum()))
    rec = dict(case=case["name"], variant=variant, n0=len(res["up"]), n_spawn=len(sp["up"]), joins=want["joins"])
    try:
        EC._upload(g, res)
        status, out = 0, None
        try:
            out = g.annihilate(prm, sp)
        except sqmc_amd.SqmcGpuError as e:
            status = e.code
        rec["status"] = status
        if status < 0:
            rec["ok"] = False; rec["why"] = "library failure"
            return rec
        want_status = meta.get("status", 0)
        why = None if status == want_status else "status %d, expected %d" % (status, want_status)
        if status != 1:                      # status 1 is refused at the door, in front of any tail
            tail = g.last_tail(); rec["tail"] = tail
            if tail["kind"] != "radix" or tail["merge"] or tail["packed"] != (variant != "plain_unpacked"):
                why = why or "tail %r: a plain step takes the radix tail without the spawn-only merge" % (tail,)
        if status == 0 and why is None:
            got = g.download_walkers()
            why = EC._compare(dict(want=want, want_stats=want["stats"], stat_bound=want["stat_bound"]), got, out)
            bad = AC.chain_layer(case["heads"], case["chains"], prm, got)          # what holds whatever the draws
            if bad:
                why = (why or "") + " chain layer: %r" % (bad[:3],)
            if rng_mode == 0 and g.rng_state() != want["rng"]:
                why = why or "generator %r after the call, %r after the model's %d joins" % (g.rng_state(), want["rng"], want["joins"])
            if meta.get("kind") == "carrier":
                v, counts = carrier_verdict(case, got["up"], got["dn"], got["wt"])
                rec["carriers"] = None if counts is None else {str(s): c for s, c in counts.items()}
                why = why or v
        if want_status != 0 and why is None:
            # the context still works: the same residents with one tame spawn
            EC._upload(g, res)
            sp2 = {a: v[:1].copy() for a, v in sp.items()}
            sp2["wt"] = np.abs(sp2["wt"]) * np.sign(res["wt"][0]); sp2["up"][:] = res["up"][0]; sp2["dn"][:] = res["dn"][0]
            m = AC.plain_step(res, sp2, prm, ReplayDraws() if rng_mode == 0 else None)
            out2 = g.annihilate(prm, sp2)
            got2 = g.download_walkers()
            for a in ("up", "dn", "wt", "imp_distance", "initiator"):
                if not np.array_equal(got2[a], m[a]):
                    why = "the call after status %d: %s differs from the model" % (status, a)
            if int(out2[5]) != len(m["up"]):
                why = why or "the call after status %d: nwalk" % status
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def main(argv):
    path, variant = argv[1], argv[2]
    for k, v in VARIANTS[variant][0].items():
        assert os.environ.get(k) == v, "the environment of this process does not select variant %s" % variant
    assert variant == "plain_counter_serial_join" or "SQMC_SERIAL_JOIN" not in os.environ
    with open(path, "rb") as f:
        blob = pickle.load(f)
    import sqmc_amd
    sqmc_amd.set_device(0)
    t0 = time.time()
    n_bad = 0
    for case in blob["cases"]:
        if case["meta"].get("only") and variant not in case["meta"]["only"]:
            continue
        rec = run_case(blob, variant, case)
        print(json.dumps(rec, default=str), flush=True)
        if rec.get("status", 0) < 0:
            return 3
        n_bad += 0 if rec["ok"] else 1
    print(json.dumps(dict(variant=variant, cases_failed=n_bad, seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
