// cauchy_device.h -- the Cauchy-Schwarz proposal (proposal_method CauchySchwarz) on the device.  gfx950 only.
// Textually included by sqmc_gpu.hip behind chem_device.h.
//
// Reference: off_diagonal_move_chem_cauchySchwarz (chemistry.f90:2530-4233), the live branches only: setup_orb_by_symm sets
// uniform_sampling = .false. (2526) before any move, so every `if (uniform_sampling)` arm is dead.  The tables are those of
// setup_orb_by_symm (2505-2523), built by sqmc_gpu_setup_cauchy_schwarz on the host.
//
// The reference takes the second electron and both holes of a double from the compiler's intrinsic random_number (2798, 3025,
// 3080, 3315, 3369, 3609, 3698, 3899), a stream nothing can pin.  Here every such draw is the walk's own stream at the same
// position (tests/golden/README_cauchyschwarz.md, decision 1).  A cumulative search that rounding leaves short of its draw
// ends in occ_orb(0) / ibset(det,-1) there; here it is a null move (level 0, weight 0) with the draws taken so far consumed
// (decision 2).  Arithmetic follows the reference statement by statement (no FMA contraction): left-to-right sums, x/sum per
// term, the products of proposal_prob as written.  Orbital lists are the bit masks of det_i in ascending order, which is the
// order of the reference's occ_orb_* and which_orb_by_sym lists.
#pragma once

#define CS_SQ(i, j) sq[(size_t)((i) - 1) * n + ((j) - 1)]

// cs_sqrt_prime_spin(k) of electron orbital o (chemistry.f90:2721-2727): 2 cs_sqrt_orb(o) minus sqrt_integrals(o, j) over every
// occupied orbital j, up ascending then dn ascending (core orbitals included)
__device__ __forceinline__ double cs_prime_spin(const double *__restrict__ sq, const double *__restrict__ orb, int n, int o, u64 iu, u64 id) {
  double v = 2 * orb[o - 1];
  for (u64 b = iu; b; b &= b - 1) v = v - CS_SQ(o, ctz64(b) + 1);
  for (u64 b = id; b; b &= b - 1) v = v - CS_SQ(o, ctz64(b) + 1);
  return v;
}
// cs_sqrt_prime(k) (2709-2720): cs_sqrt_orb(o) minus sqrt_integrals(o, j) over the occupied orbitals j of o's own spin
__device__ __forceinline__ double cs_prime(const double *__restrict__ sq, const double *__restrict__ orb, int n, int o, u64 own) {
  double v = orb[o - 1];
  for (u64 b = own; b; b &= b - 1) v = v - CS_SQ(o, ctz64(b) + 1);
  return v;
}
// sum over the orbitals x of `bits`, ascending, of  (acc + sqrt_integrals(o2,x)) + sqrt_integrals(o1,x)  (the "electron_prob"
// loops in front of every denominator, e.g. 3082-3085)
__device__ __forceinline__ double cs_pair_sum(const double *__restrict__ sq, int n, int o1, int o2, u64 bits) {
  double acc = 0.0;
  for (u64 b = bits; b; b &= b - 1) { const int x = ctz64(b) + 1; acc = acc + CS_SQ(o2, x) + CS_SQ(o1, x); }
  return acc;
}
// sym_sum_cs_sqrt(sym, o2) + sym_sum_cs_sqrt(sym, o1): the first two terms of every second-hole denominator
__device__ __forceinline__ double ssum_pair(const double *__restrict__ ssum, int n, int s, int o1, int o2) {
  return ssum[(size_t)(s - 1) * n + (o2 - 1)] + ssum[(size_t)(s - 1) * n + (o1 - 1)];
}
// second hole: cumulative search over the open orbitals `open` ascending with weight (sqrt(o2,x)+sqrt(o1,x))/den; 0 = fell through
__device__ __forceinline__ int cs_pick_second(const double *__restrict__ sq, int n, int o1, int o2, u64 open, double den, double r) {
  double ep = 0.0;
  for (u64 b = open; b; b &= b - 1) {
    const int x = ctz64(b) + 1;
    ep = ep + (CS_SQ(o2, x) + CS_SQ(o1, x)) / den;
    if (r <= ep) return x;
  }
  return 0;
}

// One proposal from det_i.  Returns the excitation level (1/2) with det_j and the proposal probability, or 0 (det_j = det_i)
// when the reference returns with weight 0 or a search falls through.
__device__ inline int propose_cauchy_schwarz(const ChemTab &t, const CsDev &cs, Rng &g, u64 iu, u64 id, u64 &ju, u64 &jd, double &prob) {
  const double *__restrict__ sq = cs.sq;
  const double *__restrict__ orb = cs.orb;
  const double *__restrict__ ssum = cs.sym;
  const int nup = t.nup, ndn = t.ndn, norb = t.norb, nc = t.ncore, nelec = t.nelec, n = norb;
  const int n_single = (nup - nc) * (norb - nup) + (ndn - nc) * (norb - ndn);
  const int n_double_up = (nup - nc) * (nup - nc - 1) * (norb - nup) * (norb - nup - 1) / 4;
  const int n_double_dn = (ndn - nc) * (ndn - nc - 1) * (norb - ndn) * (norb - ndn - 1) / 4;
  const int n_double_both = (nup - nc) * (norb - nup) * (ndn - nc) * (norb - ndn);
  const int n_double = n_double_up + n_double_dn + n_double_both, n_total = n_single + n_double;
  prob = 1.0;
  ju = iu; jd = id;
  if (rng_int(g, n_total) <= n_single) {
    // single excitation: electron and hole by random_int, as in uniform2 (2886-2985)
    prob = prob * n_single / (n_total * 1.0);
    int e = rng_int(g, nelec - 2 * nc);
    const bool up = !(e > nup - nc);
    const u64 d = up ? iu : id;
    const int o = kth_set(d, up ? e + nc : e + 2 * nc - nup);
    const int sym1 = t.orbsym[o];
    prob = prob / (nelec - 2 * nc);
    const u64 open = t.sym_mask[sym1] & ~d;
    const int i_open = popc64(open);
    if (i_open == 0) return 0;
    const int to1 = rng_int(g, i_open); prob = prob / i_open;
    const int h = kth_set_wide(open, to1);
    if (up) { ju = (iu & ~bit64(o - 1)) | bit64(h - 1); } else { jd = (id & ~bit64(o - 1)) | bit64(h - 1); }
    return 1;
  }
  prob = n_double / (double)n_total;
  // the active electrons: det_i without its n_core_orb lowest orbitals of each spin
  u64 au = iu, ad = id;
  for (int q = 0; q < nc; q++) { au &= au - 1; ad &= ad - 1; }
  // first electron (2729-2762): cumulative search over cs_sqrt_prime_spin / sum_cs_sqrt_prime, up electrons first
  double ssp = 0.0;
  for (u64 b = au; b; b &= b - 1) ssp = ssp + cs_prime_spin(sq, orb, n, ctz64(b) + 1, iu, id);
  for (u64 b = ad; b; b &= b - 1) ssp = ssp + cs_prime_spin(sq, orb, n, ctz64(b) + 1, iu, id);
  int o1 = 0; bool up1 = false; double c1 = 0.0;
  {
    const double r = rng_draw(g);
    double ep = 0.0;
    for (u64 b = au; b && !o1; b &= b - 1) {
      const int o = ctz64(b) + 1; const double v = cs_prime_spin(sq, orb, n, o, iu, id);
      ep = ep + v / ssp;
      if (r <= ep) { o1 = o; up1 = true; c1 = v; }
    }
    for (u64 b = ad; b && !o1; b &= b - 1) {
      const int o = ctz64(b) + 1; const double v = cs_prime_spin(sq, orb, n, o, iu, id);
      ep = ep + v / ssp;
      if (r <= ep) { o1 = o; up1 = false; c1 = v; }
    }
    if (!o1) return 0;
  }
  // second electron (2798-2850): the same search without the first one
  int o2 = 0; bool up2 = false; double c2 = 0.0;
  {
    const double r = rng_draw(g);
    const double rest = ssp - c1;
    double ep = 0.0;
    for (u64 b = au; b && !o2; b &= b - 1) {
      const int o = ctz64(b) + 1;
      if (up1 && o == o1) continue;
      const double v = cs_prime_spin(sq, orb, n, o, iu, id);
      ep = ep + v / rest;
      if (r <= ep) { o2 = o; up2 = true; c2 = v; }
    }
    for (u64 b = ad; b && !o2; b &= b - 1) {
      const int o = ctz64(b) + 1;
      if (!up1 && o == o1) continue;
      const double v = cs_prime_spin(sq, orb, n, o, iu, id);
      ep = ep + v / rest;
      if (r <= ep) { o2 = o; up2 = false; c2 = v; }
    }
    if (!o2) return 0;
  }
  // 2857-2860: both orders in which the pair could have been drawn
  prob = prob * (c1 / ssp * c2 / (ssp - c1) + c2 / ssp * c1 / (ssp - c2));
  // the pair in occ_orb order (2904-2906): up before dn, ascending inside a spin
  if ((up1 == up2 && o1 > o2) || (!up1 && up2)) {
    const int to = o1; o1 = o2; o2 = to; const bool tu = up1; up1 = up2; up2 = tu;
  }
  if (up1) ju &= ~bit64(o1 - 1); else jd &= ~bit64(o1 - 1);
  if (up2) ju &= ~bit64(o2 - 1); else jd &= ~bit64(o2 - 1);
  const int sym1 = t.prod[t.orbsym[o1]][t.orbsym[o2]];
  if (up1 == up2) {
    // both electrons of one spin (tot_spin_from = +-2, 3015-3307 and 3308-3600)
    const bool up = up1;
    const u64 d = up ? iu : id;
    const double den1 = cs_prime(sq, orb, n, o1, d) + cs_prime(sq, orb, n, o2, d);
    int h1 = 0;
    {
      const double r = rng_draw(g);
      double ep = 0.0;
      for (u64 b = t.orb_mask & ~d; b; b &= b - 1) {
        const int x = ctz64(b) + 1;
        ep = ep + (CS_SQ(o1, x) + CS_SQ(o2, x)) / den1;
        if (r <= ep) { h1 = x; break; }
      }
    }
    if (!h1) { ju = iu; jd = id; return 0; }
    const int s1 = t.orbsym[h1];
    const int sym2 = t.prod[s1][sym1];
    const bool same = (sym2 == s1);
    const u64 occ2 = (t.sym_mask[sym2] & d) | (same ? bit64(h1 - 1) : 0ull);      // occ_orb_*_by_sym(_copy)(sym2, :)
    const u64 open2 = t.sym_mask[sym2] & ~occ2;
    if (popc64(open2) == 0) { ju = iu; jd = id; return 0; }
    const double r = rng_draw(g);
    double den = ssum[(size_t)(sym2 - 1) * n + (o2 - 1)] + ssum[(size_t)(sym2 - 1) * n + (o1 - 1)] - cs_pair_sum(sq, n, o1, o2, occ2);
    const int h2 = cs_pick_second(sq, n, o1, o2, open2, den, r);
    if (!h2) { ju = iu; jd = id; return 0; }
    if (up) ju |= bit64(h1 - 1) | bit64(h2 - 1); else jd |= bit64(h1 - 1) | bit64(h2 - 1);
    double temp = (CS_SQ(o1, h1) + CS_SQ(o2, h1)) / den1 * (CS_SQ(o2, h2) + CS_SQ(o1, h2)) / den;
    if (same) {
      den = den + CS_SQ(o2, h1) - CS_SQ(o2, h2) + CS_SQ(o1, h1) - CS_SQ(o1, h2);
    } else {
      den = ssum[(size_t)(s1 - 1) * n + (o2 - 1)] + ssum[(size_t)(s1 - 1) * n + (o1 - 1)] - cs_pair_sum(sq, n, o1, o2, t.sym_mask[s1] & d);
    }
    temp = temp + (CS_SQ(o1, h2) + CS_SQ(o2, h2)) / den1 * (CS_SQ(o2, h1) + CS_SQ(o1, h1)) / den;
    prob = prob * temp;
    return 2;
  }
  // one up and one dn electron (3601-4200): the first hole among the empty up orbitals, then the empty dn orbitals
  const double den1 = cs_prime_spin(sq, orb, n, o1, iu, id) + cs_prime_spin(sq, orb, n, o2, iu, id);
  int h1 = 0; bool hup = true;
  {
    const double r = rng_draw(g);
    double ep = 0.0;
    for (u64 b = t.orb_mask & ~iu; b && !h1; b &= b - 1) {
      const int x = ctz64(b) + 1;
      ep = ep + (CS_SQ(o1, x) + CS_SQ(o2, x)) / den1;
      if (r <= ep) { h1 = x; hup = true; }
    }
    for (u64 b = t.orb_mask & ~id; b && !h1; b &= b - 1) {
      const int x = ctz64(b) + 1;
      ep = ep + (CS_SQ(o1, x) + CS_SQ(o2, x)) / den1;
      if (r <= ep) { h1 = x; hup = false; }
    }
  }
  if (!h1) { ju = iu; jd = id; return 0; }
  const u64 d1 = hup ? iu : id, d2 = hup ? id : iu;          // strings of the first and of the second hole
  const int s1 = t.orbsym[h1];
  const int sym2 = t.prod[sym1][s1];
  const u64 open2 = t.sym_mask[sym2] & ~d2;
  if (popc64(open2) == 0) { ju = iu; jd = id; return 0; }
  const double r = rng_draw(g);
  const double den = ssum[(size_t)(sym2 - 1) * n + (o2 - 1)] + ssum[(size_t)(sym2 - 1) * n + (o1 - 1)] - cs_pair_sum(sq, n, o1, o2, t.sym_mask[sym2] & d2);
  const int h2 = cs_pick_second(sq, n, o1, o2, open2, den, r);
  if (!h2) { ju = iu; jd = id; return 0; }
  if (hup) { ju |= bit64(h1 - 1); jd |= bit64(h2 - 1); } else { jd |= bit64(h1 - 1); ju |= bit64(h2 - 1); }
  double temp = (CS_SQ(o1, h1) + CS_SQ(o2, h1)) / den1 * (CS_SQ(o2, h2) + CS_SQ(o1, h2)) / den;
  if (popc64(t.sym_mask[s1] & ~d1) != 0) {        // always: h1 itself is open
    const double den3 = ssum[(size_t)(s1 - 1) * n + (o2 - 1)] + ssum[(size_t)(s1 - 1) * n + (o1 - 1)] - cs_pair_sum(sq, n, o1, o2, t.sym_mask[s1] & d1);
    temp = temp + (CS_SQ(o1, h2) + CS_SQ(o2, h2)) / den1 * (CS_SQ(o2, h1) + CS_SQ(o1, h1)) / den3;
  }
  prob = prob * temp;
  return 2;
}
#undef CS_SQ

// ---------------------------------------------------------------------------------------------------- time-reversal symmetry
// The Cauchy-Schwarz arm of is_connected_chem (chemistry.f90:2203-2450; singles: the uniform formula, 2131-2152) for det_i -> target:
// the excitation level and the probability of the move reaching the target, without the n_single / n_total or n_double / n_total
// factor.  As the product means it (tests/golden/README_cauchyschwarz_time_sym.md): the move tables are det_i's own, computed here
// (the reference reads module state the move fills only on its double branch, item 2), and the up-up second path sums with `+`
// (2288 has `-`, item 1).  Operation order otherwise that of the text.  Draws nothing.
#define CS_SQ(i, j) sq[(size_t)((i) - 1) * n + ((j) - 1)]
#define CS_SYM(s, o) ssum[(size_t)((s) - 1) * n + ((o) - 1)]
__device__ inline bool cs_is_connected_prob(const ChemTab &t, const CsDev &cs, u64 iu, u64 id, u64 ju, u64 jd, int &level, double &prob) {
  const double *__restrict__ sq = cs.sq;
  const double *__restrict__ orb = cs.orb;
  const double *__restrict__ ssum = cs.sym;
  const int n = t.norb;
  int upc = 0, dnc = 0, du1 = 0, du2 = 0, du3 = 0, du4 = 0, dd1 = 0, dd2 = 0, dd3 = 0, dd4 = 0;
  level = -1; prob = 0.0;
  if (iu != ju) {
    const u64 a = iu & ~ju, b = ju & ~iu;
    upc = popc64(a);
    if (upc > 2 || upc != popc64(b)) return false;
    du1 = ctz64(a) + 1; du3 = ctz64(b) + 1;
    if (upc == 2) { du2 = ctz64(a & (a - 1)) + 1; du4 = ctz64(b & (b - 1)) + 1; }
  }
  if (id != jd) {
    const u64 a = id & ~jd, b = jd & ~id;
    dnc = popc64(a);
    if (dnc > 2 || dnc != popc64(b)) return false;
    dd1 = ctz64(a) + 1; dd3 = ctz64(b) + 1;
    if (dnc == 2) { dd2 = ctz64(a & (a - 1)) + 1; dd4 = ctz64(b & (b - 1)) + 1; }
  }
  level = upc + dnc;
  if (level > 2) { level = -1; return false; }
  const int ne = t.nelec - 2 * t.ncore;
  if (level == 1) {
    u64 det = id; int d1 = dd1, d2 = dd3;
    if (upc == 1) { det = iu; d1 = du1; d2 = du3; }
    const int sym1 = t.orbsym[d1];
    if (sym1 != t.orbsym[d2]) return false;
    const int i_open = popc64(t.sym_mask[sym1] & ~det);
    prob = 1.0 / ((ne) * (i_open));
    return true;
  }
  if (level != 2) return true;
  int o1, o2, k, l;
  if (upc == 2) { o1 = du1; o2 = du2; k = du3; l = du4; }
  else if (dnc == 2) { o1 = dd1; o2 = dd2; k = dd3; l = dd4; }
  else { o1 = du1; o2 = dd1; k = du3; l = dd3; }
  if (t.prod[t.orbsym[o1]][t.orbsym[o2]] != t.prod[t.orbsym[k]][t.orbsym[l]]) return false;
  // sum_cs_sqrt_prime of det_i (2729-2737): active up electrons, then active dn electrons
  u64 au = iu, ad = id;
  for (int q = 0; q < t.ncore; q++) { au &= au - 1; ad &= ad - 1; }
  double s = 0.0;
  for (u64 b = au; b; b &= b - 1) s = s + cs_prime_spin(sq, orb, n, ctz64(b) + 1, iu, id);
  for (u64 b = ad; b; b &= b - 1) s = s + cs_prime_spin(sq, orb, n, ctz64(b) + 1, iu, id);
  const double c1 = cs_prime_spin(sq, orb, n, o1, iu, id), c2 = cs_prime_spin(sq, orb, n, o2, iu, id);
  const double pp = (c1 / s * c2 / (s - c1) + c2 / s * c1 / (s - c2));
  double tmp;
  if (upc == 2 || dnc == 2) {
    // both electrons of one spin (2220-2375); i_open is never 0 (l, and k, are open), the tests are the text's
    const u64 own = (upc == 2) ? iu : id;
    int sym1 = t.orbsym[l];
    int i_open = popc64(t.sym_mask[sym1] & ~own) - (sym1 == t.orbsym[k] ? 1 : 0);
    if (i_open == 0) return true;
    double den = ssum_pair(ssum, n, sym1, o1, o2) - cs_pair_sum(sq, n, o1, o2, t.sym_mask[sym1] & own);
    if (sym1 == t.orbsym[k]) den = den - CS_SQ(o2, k) - CS_SQ(o1, k);
    const double den1 = cs_prime(sq, orb, n, o1, own) + cs_prime(sq, orb, n, o2, own);
    tmp = (CS_SQ(o1, k) + CS_SQ(o2, k)) / den1 * (CS_SQ(o2, l) + CS_SQ(o1, l)) / den;
    sym1 = t.orbsym[k];
    i_open = popc64(t.sym_mask[sym1] & ~own) - (sym1 == t.orbsym[l] ? 1 : 0);
    if (i_open != 0) {
      if (sym1 == t.orbsym[l]) den = den + CS_SQ(o2, k) - CS_SQ(o2, l) + CS_SQ(o1, k) - CS_SQ(o1, l);
      else den = ssum_pair(ssum, n, sym1, o1, o2) - cs_pair_sum(sq, n, o1, o2, t.sym_mask[sym1] & own);
      tmp = tmp + (CS_SQ(o1, l) + CS_SQ(o2, l)) / den1 * (CS_SQ(o2, k) + CS_SQ(o1, k)) / den;
    }
  } else {
    // one up and one dn electron (2376-2444)
    int sym1 = t.orbsym[l];
    if (popc64(t.sym_mask[sym1] & ~id) == 0) return true;
    double den = ssum_pair(ssum, n, sym1, o1, o2) - cs_pair_sum(sq, n, o1, o2, t.sym_mask[sym1] & id);
    const double den1 = c1 + c2;
    tmp = (CS_SQ(o1, k) + CS_SQ(o2, k)) / den1 * (CS_SQ(o2, l) + CS_SQ(o1, l)) / den;
    sym1 = t.orbsym[k];
    if (popc64(t.sym_mask[sym1] & ~iu) != 0) {
      den = ssum_pair(ssum, n, sym1, o1, o2) - cs_pair_sum(sq, n, o1, o2, t.sym_mask[sym1] & iu);
      tmp = tmp + (CS_SQ(o1, l) + CS_SQ(o2, l)) / den1 * (CS_SQ(o2, k) + CS_SQ(o1, k)) / den;
    }
  }
  prob = pp * tmp;
  return true;
}
#undef CS_SYM
#undef CS_SQ

// weight_j of a Cauchy-Schwarz proposal det_i -> det_j (level, prob).  time_sym: the end of off_diagonal_move_chem_cauchySchwarz
// (4093-4162) -- proposal_weight's time-symmetric branch, but for det_j with up == dn (z = 1) the probability and norm_j are
// rescaled by the arm's value for det_j itself (4098-4108) -- the second pathway through flip(det_j) from cs_is_connected_prob, and
// det_j replaced by its representative.  The walk runs it in a kernel of its own (SPAWN_CAUCHY_TS): inlined there, out of the plain
// Cauchy-Schwarz kernel.
__device__ inline double cs_time_sym_weight(const ChemTab &t, const CsDev &cs, const double *__restrict__ ints, double tau, u64 iu, u64 id, u64 &ju,
                                                  u64 &jd, int level, double prob) {
  const double sqrt2 = sqrt(2.0);
  const double norm_i = (iu == id) ? sqrt2 : 1.0;
  if ((ju == iu && jd == id) || (jd == iu && ju == id)) return 0.0;
  const int nup = t.nup, ndn = t.ndn, norb = t.norb, nc = t.ncore;
  const int n_single = (nup - nc) * (norb - nup) + (ndn - nc) * (norb - ndn);
  const int n_double = (nup - nc) * (nup - nc - 1) * (norb - nup) * (norb - nup - 1) / 4 + (ndn - nc) * (ndn - nc - 1) * (norb - ndn) * (norb - ndn - 1) / 4
                     + (nup - nc) * (norb - nup) * (ndn - nc) * (norb - ndn);
  const int n_total = n_single + n_double;
  int lsym; double psym;
  double me;
  if (ju == jd) {
    if (t.z != 1) return 0.0;
    cs_is_connected_prob(t, cs, iu, id, jd, ju, lsym, psym);
    double norm_j = 1 / prob;
    if (lsym == 1) prob = (prob + psym * (n_single / (double)n_total)) / 2;
    else prob = (prob + psym * (n_double / (double)n_total)) / 2;
    norm_j = 2 * norm_j / sqrt2 * (prob);
    me = h_level(t, ints, iu, id, ju, jd, level);
    me = (norm_j / norm_i) * me;
  } else {
    const double m1 = h_level(t, ints, iu, id, ju, jd, level);
    if (cs_is_connected_prob(t, cs, iu, id, jd, ju, lsym, psym)) {
      const double m2 = h_level(t, ints, iu, id, jd, ju, lsym);
      if (lsym == 1) prob = prob + (psym * (n_single / (double)n_total));
      if (lsym == 2) prob = prob + (psym * (n_double / (double)n_total));
      me = (1.0 / norm_i) * (m1 + t.z * m2);
    } else me = (1.0 / norm_i) * (m1);
  }
  if (ju > jd) { const u64 x = ju; ju = jd; jd = x; me = me * t.z; }
  return -tau * me / prob;
}
__device__ __forceinline__ double cs_proposal_weight(const ChemTab &t, const CsDev &cs, const double *__restrict__ ints, double tau, u64 iu, u64 id, u64 &ju,
                                                     u64 &jd, int level, double prob) {
  if (!t.time_sym) return -tau * h_level(t, ints, iu, id, ju, jd, level) / prob;
  return cs_time_sym_weight(t, cs, ints, tau, iu, id, ju, jd, level, prob);
}
