"""An independent model of the plane-wave Hubbard model in its symmetry-adapted basis (hubbardk with space_sym), on top of
tests/hubbardk_checker.py and of nothing from oracle/ or the HIP library.

The group is C4 x reflection x spin inversion, 16 elements g = Z^s P^f R^r (R^r first):
  R: (kx, ky) -> (ky, -kx),  P: (kx, ky) -> (-ky, -kx),  Z: up <-> dn,
momenta folded modulo 2 l.  Each element acts on a second-quantised state a+_{P1} a+_{P2} ... |0> (spin orbitals ascending, up before
dn) as the signed permutation a+_{g P1} a+_{g P2} ... |0>: the sign is the parity of the inversions of (g P1, g P2, ...).  One
convention: Z carries the constant factor (-1)^(nup ndn), so that it exchanges the two strings without a sign (a constant times a
symmetry is a symmetry; for two electrons z = 1 is then the singlet).  The sector is the one-dimensional representation
chi(g) = z^s p^f (C4-A1), its projector (1/16) sum_g chi(g) g.  A determinant's orbit vector is sum_g chi(g) g |det>; where it does not
vanish, its normalised form with a positive coefficient on the orbit's smallest determinant (the representative) is a column of V,
and the model's matrix is M = V^T A V with A the plain Hamiltonian on the momentum-0 sector.  No list of 'distinct images' is kept
anywhere: duplicates simply add up in the orbit vector."""
import math

import numpy as np

from tests import proposal_checker as PC
from tests import hubbardk_checker as HK


class Group:
    def __init__(self, H, nup, ndn, z, p):
        assert H.l_x == H.l_y and H.l_x % 2 == 0 and nup == ndn and abs(z) == 1 and abs(p) == 1
        self.H, self.n, self.nup, self.ndn, self.z, self.p = H, H.norb, nup, ndn, z, p
        n = self.n
        rot = [H.index[H.fold((k[1], -k[0]))] for k in H.k]
        ref = [H.index[H.fold((-k[1], -k[0]))] for k in H.k]
        spatial = lambda m: [m[P % n] + (P // n) * n for P in range(2 * n)]
        R, Pm, Z = spatial(rot), spatial(ref), [(P + n) % (2 * n) for P in range(2 * n)]
        ident = list(range(2 * n))
        comp = lambda a, b: [a[b[P]] for P in range(2 * n)]                 # a after b
        self.elements = []                                                    # index k = r + 4 s + 8 f: (spin-orbital map, character, constant)
        for f in (0, 1):
            for s in (0, 1):
                Rr = ident
                for r in range(4):
                    m = comp(Z, comp(Pm, Rr)) if (s and f) else comp(Z, Rr) if s else comp(Pm, Rr) if f else Rr
                    const = (-1) ** (nup * ndn) if s else 1
                    self.elements.append((m, (z if s else 1) * (p if f else 1), const))
                    Rr = comp(R, Rr)
        self.rot0, self.ref0 = rot, ref

    def act(self, m, det):
        """(image determinant, sign) of the signed permutation m on |det>"""
        n = self.n
        occ = PC._bits(det[0]) + [n + o for o in PC._bits(det[1])]
        img = [m[P] for P in occ]
        inv = sum(1 for a in range(len(img)) for b in range(a + 1, len(img)) if img[a] > img[b])
        up = sum(1 << q for q in img if q < n)
        dn = sum(1 << (q - n) for q in img if q >= n)
        return (up, dn), (-1 if inv & 1 else 1)

    def images(self, det):
        """[(image, phase)] for the 16 elements, phase = chi(g) x the sign of g on |det>"""
        out = []
        for m, chi, const in self.elements:
            d, sg = self.act(m, det)
            out.append((d, chi * const * sg))
        return out

    def reduce(self, det):
        """(images, phases, representative, phase_w_rep, norm, num_distinct): the representative is the smallest image, phase_w_rep
        the phase of the first image equal to it, norm^2 the sum of the phases of the images equal to det"""
        im = self.images(det)
        rep = min(d for d, _ in im)
        pw = next(ph for d, ph in im if d == rep)
        norm2 = sum(ph for d, ph in im if d == det)
        return [d for d, _ in im], [ph for _, ph in im], rep, pw, math.sqrt(abs(norm2)), (int(round(16.0 / norm2)) if norm2 > 0 else 0)

    def maps_one_based(self):
        """c4_map[nsites][3] and reflection_map[nsites], 1-based, as the library's entry takes them"""
        n, r1 = self.n, self.rot0
        r2 = [r1[r1[i]] for i in range(n)]
        r3 = [r1[r2[i]] for i in range(n)]
        return [[r1[i] + 1, r2[i] + 1, r3[i] + 1] for i in range(n)], [self.ref0[i] + 1 for i in range(n)]


class Sector:
    """dets: the plain momentum-0 sector (sorted); A: the plain matrix; reps: every orbit's representative (sorted); live: those whose
    orbit vector does not vanish; V: their orthonormal orbit vectors; M = V^T A V"""

    def __init__(self, H, nup, ndn, z, p, dets=None, A=None):
        self.H, self.G = H, Group(H, nup, ndn, z, p)
        self.dets = dets if dets is not None else HK.sector(H, nup, ndn, (0, 0))
        self.A = A if A is not None else HK.dense(H, self.dets, lambda u, d: HK.excitations_hubbardk(H, u, d))
        idx = {d: i for i, d in enumerate(self.dets)}
        self.rep_of, vec = {}, {}
        for d in self.dets:
            im = self.G.images(d)
            self.rep_of[d] = min(x for x, _ in im)
        self.reps = sorted(set(self.rep_of.values()))
        cols = []
        self.live = []
        for r in self.reps:
            v = np.zeros(len(self.dets))
            for d, ph in self.G.images(r):
                v[idx[d]] += ph
            if np.any(v != 0.0):
                assert v[idx[r]] > 0
                self.live.append(r)
                cols.append(v / np.linalg.norm(v))
        self.V = np.array(cols).T if cols else np.zeros((len(self.dets), 0))
        self.M = self.V.T @ self.A @ self.V
        self.pos = {r: i for i, r in enumerate(self.live)}

    def is_live(self, det):
        return self.rep_of[det] in self.pos

    def element(self, bra, ket):
        """between orbit states; a determinant stands for its representative, 0 with a vanishing orbit"""
        a, b = self.rep_of[bra], self.rep_of[ket]
        if a not in self.pos or b not in self.pos:
            return 0.0
        return float(self.M[self.pos[a], self.pos[b]])

    def move(self, parent, child, tau):
        """the modelled move from the representative `parent` along one triple whose raw child is `child` (None: blocked):
        (determinant returned, weight).  The child is replaced by its representative; weight = -tau M[j, i] N / n_orbit, N the number of
        triples and n_orbit the number of distinct raw children of the parent in the child's orbit (each comes from one triple, so the
        triples into one orbit carry -tau M[j, i] in all); 0 for a blocked triple, a vanishing orbit, or the parent's own orbit."""
        if child is None:
            return parent, 0.0
        j = self.rep_of[child]
        if j not in self.pos or j == parent:
            return j, 0.0
        kids = HK.excitations_hubbardk(self.H, *parent)
        n_orbit = sum(1 for c in kids if self.rep_of[c] == j)
        n_triples = self.G.nup * self.G.ndn * (self.H.norb - self.G.nup)
        return j, -tau * self.element(j, parent) * n_triples / n_orbit

    def connections(self, refs, coeffs, diag_mode):
        """{representative: sum_i X[:, i] c_i} over its support, X = M (diag_mode 1) or M without the plain diagonal H_ii of each source
        (diag_mode 0: the source's own slot then holds only the terms of the symmetrised H_ii that come from its orbit), sources
        with c == 0 left out; the support: every source's own slot and every live orbit one of its raw children falls into"""
        out = {}
        for r, c in zip(refs, coeffs):
            if c == 0.0:
                continue
            plain = self.H.element(r[0], r[1], r[0], r[1])[0]
            out[r] = out.get(r, 0.0) + (self.element(r, r) - (0.0 if diag_mode == 1 else plain)) * c
            orbits = {self.rep_of[k] for k in HK.excitations_hubbardk(self.H, *r)}
            for j in orbits:
                if j in self.pos and j != r:
                    out[j] = out.get(j, 0.0) + self.element(j, r) * c
        return out
