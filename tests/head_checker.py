"""An independent model of the head of a walk step -- the spawn gate, who proposes each child, from which position of the random
stream, with which share of the weight, into which slot and with which flags -- CPU only.

Written from the reference's text: the gate of move_uniform2 (do_walk.f90:3574-3589) and what a spawned walker carries
(3700-3731).  Not from the kernels: the model has no child offsets, no search and no scan.  The parent of every child is
np.repeat of the counts; the move itself is a black box (the oracle's orc_off_diagonal_move_chem, its heat-bath move and
orc_off_diagonal_move_heg, which other tests hold bit for bit to the proposal kernels and to an independent H).

The draws come from the generator alone (Counter / Replay below): COUNTER seeks stage 0 at the determinant's rank for the gate
and stage 1 at the child's number for child c, with Rng.step the step number; REPLAY is the one rannyu stream in walker order
(a walker's gate draw, then its children's proposals, then the next walker).

layout() is the only part that restates the kernels: where k_spawn, the scan and gate_block_parents meet each child.  It serves
to assert that a case reaches the seam it is named for, and to report; the constants come from the sources (kernel_constants).
Its search, run with none of the deliberate mistakes, must give np.repeat's parents -- tests/test_head_checker.py asserts it.

Deliberate mistakes (keyword switches; test_head_checker shows a named case that notices each):
  nint_half_to_even              the gate rounds halves to even
  wchild_divides_below_cutoff    the one child of a walker below the cutoff carries w / 1, not +-cutoff
  parent_last_of_ties_wrong      a child's parent is the FIRST index of an equal-offset run, not the last
  window_edge_off_by_one         a child that is the first of the parent on the LDS window's last entry stays inside the window
  hint_block_start_exclusive     gate_block_parents skips the block that starts exactly on a parent's first child: its word is stale
  flags_of_previous_parent       a record takes imp_distance / initiator of the walker in front of its parent
  heatbath_slots_swapped         the two records of a heat-bath child change places
"""
import ctypes as C
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """TPB, SPAWN_WIN and the scan's tiles as the kernels are compiled with them"""
    csrc = os.path.join(ROOT, "sqmc_amd", "csrc")
    g = lambda name, f: int(re.search(r"#define %s \(?(\d+)" % name, open(os.path.join(csrc, f)).read()).group(1))
    sb = g("SCAN_BLOCK", "scan_sort.h")
    large = re.search(r"#define SCAN_LARGE_N \(1ll << (\d+)\)", open(os.path.join(csrc, "scan_sort.h")).read())
    return dict(TPB=g("TPB", "sqmc_gpu.hip"), SPAWN_WIN=g("SPAWN_WIN", "sqmc_gpu.hip"), SCAN_TILE=sb * g("SCAN_ITEMS_SMALL", "scan_sort.h"),
                SCAN_TILE_LARGE=sb * g("SCAN_ITEMS_LARGE", "scan_sort.h"), SCAN_LARGE_N=1 << int(large.group(1)))


# ------------------------------------------------------------------------------------------------ the generator
def _lib(O):
    L = O.lib()
    L.orc_det_rank.restype = C.c_uint64
    L.orc_det_rank.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    L.orc_rng_set_mode.argtypes = [C.c_void_p, C.c_int]
    return L


class Counter:
    """COUNTER: every draw's stream is keyed -- the gate's by the determinant's rank (stage 0), a child's by its number (stage 1)"""
    mode = 1

    def __init__(self, O, seed, step, norb, ndn):
        self.L, self.norb, self.ndn = _lib(O), int(norb), int(ndn)
        self.rng = O.Rng()
        self.L.orc_setrn(C.byref(self.rng), (C.c_int * 4)(*seed))
        self.L.orc_rng_set_mode(C.byref(self.rng), 1)
        self.rng.step = int(step)
        self.ref = C.byref(self.rng)

    def gate_draw(self, up, dn):
        self.L.orc_rng_seek(self.ref, 0, self.L.orc_det_rank(self.norb, self.ndn, int(up), int(dn)))
        return self.L.orc_rannyu(self.ref)

    def child(self, c):
        self.L.orc_rng_seek(self.ref, 1, int(c))
        return self.ref


class Replay:
    """REPLAY: one rannyu stream, consumed in walker order"""
    mode = 0

    def __init__(self, O, seed, state=None):
        self.L = _lib(O)
        self.rng = O.Rng()
        self.L.orc_setrn(C.byref(self.rng), (C.c_int * 4)(*(state if state is not None else seed)))
        self.L.orc_rng_set_mode(C.byref(self.rng), 0)
        self.ref = C.byref(self.rng)

    def gate_draw(self, up, dn):
        return self.L.orc_rannyu(self.ref)

    def child(self, c):
        return self.ref

    def state(self):
        return [int(self.rng.l[k]) for k in range(4)]


# ------------------------------------------------------------------------------------------------ the moves (black boxes)
def chem_mover(O, sysm):
    L = O.lib()
    ju, jd, wj, nd = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_int()
    a = (C.byref(ju), C.byref(jd), C.byref(wj), C.byref(nd))
    f, h = L.orc_off_diagonal_move_chem, sysm.h

    def move(ref, tau, up, dn):
        f(h, ref, tau, up, dn, *a)
        return ((ju.value, jd.value, wj.value),)
    move.slots = 1
    return move


def heg_mover(O, hsys):
    L = O.lib()
    ju, jd, wj, nd = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_int()
    a = (C.byref(ju), C.byref(jd), C.byref(wj), C.byref(nd))
    f, h = L.orc_off_diagonal_move_heg, hsys.h

    def move(ref, tau, up, dn):
        f(h, ref, tau, up, dn, *a)
        return ((ju.value, jd.value, wj.value),)
    move.slots = 1
    return move


def heatbath_mover(O, hb):
    """HeatBath.move's call with both slots kept as the reference fills them (a weight of 0: no walker on that slot)"""
    ju, jd, wj, lev, nd = (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), (C.c_double * 2)(), (C.c_int * 2)(), C.c_int()
    f, hs, hh = hb.L.orc_off_diagonal_move_chem_heatbath, hb.sysm.h, hb.h

    def move(ref, tau, up, dn):
        wj[0] = wj[1] = 0.0
        f(hs, hh, ref, tau, up, dn, ju, jd, wj, lev, C.byref(nd))
        return ((ju[0], jd[0], wj[0]), (ju[1], jd[1], wj[1]))
    move.slots = 2
    return move


# ------------------------------------------------------------------------------------------------ the gate
def nint(a, half_to_even=False):
    """Fortran's nint of a non-negative double below 2^52: halves away from zero.  floor and the difference are exact."""
    f = math.floor(a)
    d = a - f
    if d > 0.5 or (d == 0.5 and (not half_to_even or f % 2 == 1)):
        f += 1
    return int(f)


def gate_one(w, cutoff, draw, nint_half_to_even=False, wchild_divides_below_cutoff=False):
    """do_walk.f90:3577-3593 for one walker; draw() is asked only below the cutoff.  Returns (nchild, wchild)."""
    if abs(w) < cutoff:
        if draw() < abs(w / cutoff):
            return 1, (w / 1 if wchild_divides_below_cutoff else math.copysign(cutoff, w))
        return 0, 0.0
    n = max(nint(abs(w), nint_half_to_even), 1)
    return n, w / n


def gate(walkers, params, draw, **mistakes):
    """nchild, wchild of every walker; draw(i): the gate's random number of walker i (asked in walker order, only below the cutoff)"""
    wt = np.asarray(walkers["wt"], np.float64).tolist()
    cutoff = float(params["always_spawn_cutoff_wt"])
    n = len(wt)
    nchild, wchild = np.zeros(n, np.int64), np.zeros(n)
    for i, w in enumerate(wt):
        nchild[i], wchild[i] = gate_one(w, cutoff, lambda: draw(i), **mistakes)
    return nchild, wchild


def parents(nchild, consts=None, hint=False, **mistakes):
    """the parent of every child in creation order.  With a deliberate mistake: what k_spawn's search, so mistaken, would find."""
    nchild = np.asarray(nchild, np.int64)
    if not any(mistakes.values()):
        return np.repeat(np.arange(len(nchild), dtype=np.int64), nchild)
    return search(nchild, consts or kernel_constants(), hint=hint, **mistakes)["parent"]


# ------------------------------------------------------------------------------------------------ what a spawn carries
def records(walkers, params, par, wchild, moves, slots=1, flags_of_previous_parent=False, heatbath_slots_swapped=False):
    """do_walk.f90:3700-3731.  par: parent per child; moves: (ju, jd, weight_j) arrays of slots x children entries in slot order.
    Returns dict(up, dn, wt, imp_distance, initiator) per slot; a weight of 0 means no walker, and only that weight counts."""
    ju, jd, wj = (np.asarray(m) for m in moves)
    par = np.repeat(np.asarray(par, np.int64), slots)
    if heatbath_slots_swapped:
        sw = np.arange(len(par)) ^ 1
        ju, jd, wj = ju[sw], jd[sw], wj[sw]
    fl = np.maximum(par - 1, 0) if flags_of_previous_parent else par
    pd = np.asarray(walkers["imp_distance"], np.int64)[fl]
    pi = np.asarray(walkers["initiator"], np.int64)[fl]
    cti, semi = bool(params["c_t_initiator"]), bool(params["semistochastic"])
    d = np.where(pd == -2, 1 if cti else 2, np.minimum(pd, 126) + 1)          # 3703-3713: huge(1_i1b) - 1 = 126
    ini = np.where(pi >= 2, 1, 0)                                             # 3718-3722
    if cti:
        ini = np.where(pd == -2, 1, ini)                                      # 3723
    if semi:
        d = np.where(pd == 0, -1, d)                                          # 3716
        ini = np.where(pd == 0, 1, ini)                                       # 3725
    wt = np.asarray(wchild, np.float64)[par] * wj.astype(np.float64)          # one product of two doubles, rounded once
    return dict(up=ju.astype(np.uint64), dn=jd.astype(np.uint64), wt=wt, imp_distance=d.astype(np.int8), initiator=ini.astype(np.int8))


def head(walkers, params, streams, mover, consts=None, hint=False, **mistakes):
    """gate, parents and records of one step's head.  Returns dict(nchild, wchild, parent, rec, n_children[, rng: REPLAY's state])."""
    gm = {k: mistakes[k] for k in ("nint_half_to_even", "wchild_divides_below_cutoff") if mistakes.get(k)}
    pm = {k: mistakes[k] for k in ("parent_last_of_ties_wrong", "window_edge_off_by_one", "hint_block_start_exclusive") if mistakes.get(k)}
    rm = {k: mistakes[k] for k in ("flags_of_previous_parent", "heatbath_slots_swapped") if mistakes.get(k)}
    assert set(mistakes) <= set(gm) | set(pm) | set(rm) | {k for k, v in mistakes.items() if not v}, mistakes
    up, dn = np.asarray(walkers["up"]).tolist(), np.asarray(walkers["dn"]).tolist()
    tau, slots = float(params["tau"]), mover.slots
    ju, jd, wj = [], [], []

    def propose(c, i):
        for m in mover(streams.child(c), tau, up[i], dn[i]):
            ju.append(m[0]); jd.append(m[1]); wj.append(m[2])
    if streams.mode == 1:
        nchild, wchild = gate(walkers, params, lambda i: streams.gate_draw(up[i], dn[i]), **gm)
        par = parents(nchild, consts, hint=hint, **pm)
        for c, i in enumerate(par.tolist()):
            propose(c, i)
    else:
        assert not pm, "REPLAY: a child's stream position is its place in walker order"
        wt, cutoff = np.asarray(walkers["wt"], np.float64).tolist(), float(params["always_spawn_cutoff_wt"])
        nchild, wchild, c = np.zeros(len(wt), np.int64), np.zeros(len(wt)), 0
        for i, w in enumerate(wt):
            nchild[i], wchild[i] = gate_one(w, cutoff, lambda: streams.gate_draw(up[i], dn[i]), **gm)
            for _ in range(int(nchild[i])):
                propose(c, i); c += 1
        par = parents(nchild)
    rec = records(walkers, params, par, wchild, (np.array(ju, np.uint64), np.array(jd, np.uint64), np.array(wj, np.float64)), slots, **rm)
    out = dict(nchild=nchild, wchild=wchild, parent=par, rec=rec, n_children=int(nchild.sum()))
    if streams.mode == 0:
        out["rng"] = streams.state()
    return out


def residents_after(walkers, params, hii):
    """the residents' weights in front of the merge of a step whose deterministic projector is the zero matrix with a stored diagonal:
    death / clone outside the deterministic space (3743-3793), w + (0 w + E_T tau w) inside it (2255-2325), C(T) walkers of
    distance -2 untouched.  hii: H_ii per walker."""
    w = np.asarray(walkers["wt"], np.float64)
    imp = np.asarray(walkers["imp_distance"], np.int64)
    tau, et = float(params["tau"]), float(params["e_trial"])
    f = 1.0 + tau * (et - np.asarray(hii, np.float64))
    assert (f >= 0).all()
    out = w.copy()
    live = (imp >= 1) if params["semistochastic"] else np.ones(len(w), bool)
    out[live] = w[live] * f[live]
    if params["semistochastic"]:
        d = imp == 0
        out[d] = w[d] + (0.0 * w[d] + et * tau * w[d])
    return out


# ------------------------------------------------------------------------------------------------ where the kernels meet each child
def child_offsets(nchild):
    nchild = np.asarray(nchild, np.int64)
    off = np.zeros(len(nchild), np.int64)
    np.cumsum(nchild[:-1], out=off[1:])
    return off


def block_parents(nchild, hint_block_start_exclusive=False, stale=None):
    """gate_block_parents restated: bpar[b] = the walker that owns child 256 b, for every block b with a child.  Returns (bpar, written)."""
    nchild = np.asarray(nchild, np.int64)
    off = child_offsets(nchild)
    total = int(nchild.sum())
    nb = (total + 255) >> 8
    bpar = np.full(nb, -1 if stale is None else stale, np.int64)
    written = 0
    for q0 in np.nonzero(nchild)[0].tolist():
        o, nc = int(off[q0]), int(nchild[q0])
        b = ((o + 256) >> 8) if hint_block_start_exclusive else ((o + 255) >> 8)
        while (b << 8) < o + nc:
            bpar[b] = q0; written += 1; b += 1
    return bpar, written


def search(nchild, consts, hint=False, parent_last_of_ties_wrong=False, window_edge_off_by_one=False, hint_block_start_exclusive=False):
    """k_spawn's parent search restated block by block: the 256-way narrowing (or the start from parent_hint), the LDS window of
    SPAWN_WIN offsets, the global search beyond it.  Returns dict(parent, wlo, rounds, beyond: per block; tie_probes: the most probe
    positions of one narrowing round that fell on one run of equal offsets)."""
    T, W = consts["TPB"], consts["SPAWN_WIN"]
    nchild = np.asarray(nchild, np.int64)
    n0, total = len(nchild), int(nchild.sum())
    off = child_offsets(nchild)
    nb = (total + T - 1) // T
    BIG = np.int64(2 ** 62)
    bpar = block_parents(nchild, hint_block_start_exclusive, stale=max(n0 - 1, 0))[0] if hint else None
    parent = np.zeros(total, np.int64)
    wlo_b, rounds_b, beyond_b, tie_probes = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.int64), 0
    t = np.arange(T, dtype=np.int64)
    for b in range(nb):
        c0 = b * T
        wlo, whi = 0, n0
        if hint:
            h = int(bpar[b])
            wlo = h if h < n0 else max(n0 - 1, 0)
            whi = wlo
        while whi - wlo > W:
            stepw = (whi - wlo + T - 1) // T
            probe = wlo + t * stepw
            ok = probe < whi
            pv = np.where(ok, off[np.minimum(probe, n0 - 1)], BIG)
            le = ok & (pv <= c0)
            cnt = int(le.sum())
            assert cnt >= 1
            same = pv[ok][pv[ok] == pv[cnt - 1]]
            tie_probes = max(tie_probes, len(same))
            nlo = wlo + (cnt - 1) * stepw
            whi = min(nlo + stepw, whi); wlo = nlo
            rounds_b[b] += 1
        wlo_b[b] = wlo
        idx = wlo + np.arange(W, dtype=np.int64)
        win = np.where(idx < n0, off[np.minimum(idx, n0 - 1)], BIG)
        c = np.arange(c0, min(c0 + T, total), dtype=np.int64)
        past = win[W - 1] <= c
        if window_edge_off_by_one:
            past = win[W - 1] < c
        inside = wlo + np.maximum(np.searchsorted(win[:W - 1], c, side="right") - 1, 0)
        glob = np.maximum(np.searchsorted(off, c, side="right") - 1, wlo + W - 1)
        p = np.where(past, glob, inside)
        beyond_b[b] = int(past.sum())
        parent[c0:c0 + len(c)] = p
    if parent_last_of_ties_wrong:
        first_of_run = np.searchsorted(off, off, side="left")
        parent = first_of_run[parent]
    return dict(parent=parent, wlo=wlo_b, rounds=rounds_b, beyond=beyond_b, tie_probes=tie_probes, bpar=bpar)


def layout(nchild, consts, hint=False):
    """the seams a list of child counts reaches, as numbers a case can be held to and a report can print"""
    nchild = np.asarray(nchild, np.int64)
    n0, total = len(nchild), int(nchild.sum())
    s = search(nchild, consts, hint=hint)
    childless = nchild == 0
    edges = np.flatnonzero(np.diff(np.concatenate([[0], childless.astype(np.int8), [0]])))
    longest = int((edges[1::2] - edges[::2]).max()) if len(edges) else 0
    tile = consts["SCAN_TILE_LARGE"] if n0 >= consts["SCAN_LARGE_N"] else consts["SCAN_TILE"]
    nt = (n0 + tile - 1) // tile
    sums = np.add.reduceat(nchild, np.arange(0, n0, tile)) if n0 else np.zeros(0, np.int64)
    bpar, written = block_parents(nchild)
    off = child_offsets(nchild)
    heavy = np.flatnonzero(nchild >= consts["TPB"] - 1)
    return dict(n0=n0, n_children=total, blocks=len(s["wlo"]), narrowing_rounds=int(s["rounds"].max()) if len(s["rounds"]) else 0,
                children_beyond_window=int(s["beyond"].sum()), blocks_with_beyond=int((s["beyond"] > 0).sum()), tie_probes=int(s["tie_probes"]),
                longest_childless_run=longest, scan_tile=int(tile), scan_tiles=int(nt), scan_zero_tiles=int((sums == 0).sum()),
                scan_tiles_past_2_20=int((sums > (1 << 20)).sum()), bpar_written=int(written), bpar_blocks=len(bpar),
                heavy_nchild=nchild[heavy].tolist()[:16], heavy_off_mod=(off[heavy] % consts["TPB"]).tolist()[:16], heavy_slots=heavy.tolist()[:16],
                n_children_mod=total % consts["TPB"], parents_ok=bool(np.array_equal(s["parent"], parents(nchild))))
