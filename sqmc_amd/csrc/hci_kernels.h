// hci_kernels.h -- Heat-bath CI connection generation kernels
// Textually included by sqmc_gpu.hip (one translation unit: the kernels share the ChemTab LDS
// image, the walker SoA types and the launch helpers defined there); not a standalone header.

#define HEG_LUT_MAX 729            // (2*4+1)^3: plane-wave indices up to +-4 per direction
// ================================================================ HCI connections
// find_important_connected_dets_chem, chemistry.f90:6819-7159: one thread per reference
// determinant; pass 0 counts, pass 1 writes at the scanned offsets.  Emits (up, dn,
// H_ij*c_j, e_mix_den) with the reference determinant itself in slot 0.
// A reference determinant with c == 0 emits nothing, slot 0 included: find_doubly_excited does not call the generator for
// it (semistoch.f90:1762, 1798, 1854, 1891).
// REC: every connection also carries the record get_new_diag_elem works from (diag_update.h; diag_elems_info of the reference,
// chemistry.f90:7148-7152): the source's H_ii, computed once per source before generation, and the packed p, q -> r, s of a double
// excitation; DU_NONE for the self slot and for single excitations (old_diag_elem = 1e51 there, :6898, :6990).  REC = false is
// the kernel as it always was: nothing extra is computed or written, orec_old / orec_pk are not touched.
// hubbardk (find_connected_dets_hubbard_k, hubbard.f90:5462): up electrons x dn electrons x empty up orbitals, all ascending -- the
// "generation order" of diag_mode 2 --, the dn electron to the orbital that conserves the total momentum, if it is empty.  A connection
// is kept when |H c| > eps (strict; the product itself is compared, not |H| with eps / |c|, so that a tie is a tie).  Every |H| is U / nsites, so the screen selects on |c| alone: a reference determinant keeps all
// of its connections or none.  No diagonal-update record exists for this system (the REC instantiation never gets here).  Out of line:
// k_hci_gen holds a call on this branch, and the code of the other systems' branches is what it was.
// Two calls, each with everything passed in registers and few enough of them that neither climbs past the kernel's own register count (a
// reference to a caller's local would give k_hci_gen a stack): hci_gen_hubbardk counts the connections and, given ou / od, writes the
// determinants; hci_fill_hubbardk then writes H c and e_mix_den for them (den: the source's index in raw mode, else 0).
__device__ __noinline__ u64 hci_gen_hubbardk(const ChemTab &t, const u64 *binom, u64 n_dn_strings, u64 up, u64 dn, u64 *ou, u64 *od, u64 key_lo, u64 key_hi) {
  const bool sliced = !(key_lo == 0 && key_hi == ~0ull);
  u64 cnt = 0;
#pragma nounroll
  for (u64 eu = up; eu; eu &= eu - 1) {
    const int p = ctz64(eu) + 1;
#pragma nounroll
    for (u64 ed = dn; ed; ed &= ed - 1) {
      const int q = ctz64(ed) + 1;
#pragma nounroll
      for (u64 hr = t.orb_mask & ~up; hr; hr &= hr - 1) {
        const int r = ctz64(hr) + 1;
        const int s_ = hk_orbital(t, t.krel[q][0] - (t.krel[r][0] - t.krel[p][0]), t.krel[q][1] - (t.krel[r][1] - t.krel[p][1]));
        if (!s_ || ((dn >> (s_ - 1)) & 1)) continue;
        const u64 nu = (up & ~bit64(p - 1)) | bit64(r - 1), nd = (dn & ~bit64(q - 1)) | bit64(s_ - 1);
        if (sliced) {                     // det_key, one electron at a time: few registers matter more here than loads in flight
          u64 ru = 0, rd = 0; int k = 1;
#pragma nounroll
          for (u64 d = nu; d; d &= d - 1, k++) ru += binom[ctz64(d) * SQ_BINOM_STRIDE + k];
          k = 1;
#pragma nounroll
          for (u64 d = nd; d; d &= d - 1, k++) rd += binom[ctz64(d) * SQ_BINOM_STRIDE + k];
          const u64 kk = ru * n_dn_strings + rd;
          if (!(kk >= key_lo && kk < key_hi)) continue;
        }
        if (ou) { ou[cnt] = nu; od[cnt] = nd; }      // null in the counting pass
        cnt++;
      }
    }
  }
  return cnt;
}
__device__ __noinline__ void hci_fill_hubbardk(const ChemTab &t, u64 up, u64 dn, double c, double den, const u64 *ou, const u64 *od, double *onum, double *oden, u64 cnt) {
#pragma nounroll
  for (u64 k = 0; k < cnt; k++) {
    const double mel = t.hk_ubyn * permutation_factor(up, ou[k]) * permutation_factor(dn, od[k]);
    onum[k] = mel * c; oden[k] = den;
  }
}
// hubbardk with space_sym (find_connected_dets_hubbard_k's closing block, hubbard.f90:5611-5627): the reference maps the raw connections to
// representatives, keeps each once and asks hamiltonian_hubbard_k_space_sym for its element.  Here every raw child j' is emitted as
// (representative of j',  phase_w_rep(j') norm_j / norm_i <j'|H|i> c): the raw children of i inside one orbit are that orbit's distinct images
// with an element to i, so the caller's sort-and-sum adds exactly the terms of the symmetrised element.  Raw children in the orbit of i itself
// land on i's own slot, which therefore holds the plain diagonal in diag_mode 1 (the two add up to the symmetrised H_ii, where the reference has
// those terms) and only those terms in diag_mode 0.  Children without a state in the (z, p) sector are dropped; a slice selects on the
// representative's key.  The eps screen stays what it is without space_sym, on the raw term |U / nsites c|, not on the summed element.
// The counting pass and the writing pass make the same decisions; the writing pass leaves phase_w_rep norm_j times the two permutation factors
// in onum, and hci_fill_hubbardk_sym turns it into H c.
__device__ __noinline__ u64 hci_gen_hubbardk_sym(const ChemTab &t, const u64 *binom, u64 n_dn_strings, u64 up, u64 dn, u64 *ou, u64 *od, double *onum, u64 key_lo, u64 key_hi) {
  const bool sliced = !(key_lo == 0 && key_hi == ~0ull);
  u64 cnt = 0;
#pragma nounroll
  for (u64 eu = up; eu; eu &= eu - 1) {
    const int p = ctz64(eu) + 1;
#pragma nounroll
    for (u64 ed = dn; ed; ed &= ed - 1) {
      const int q = ctz64(ed) + 1;
#pragma nounroll
      for (u64 hr = t.orb_mask & ~up; hr; hr &= hr - 1) {
        const int r = ctz64(hr) + 1;
        const int s_ = hk_orbital(t, t.krel[q][0] - (t.krel[r][0] - t.krel[p][0]), t.krel[q][1] - (t.krel[r][1] - t.krel[p][1]));
        if (!s_ || ((dn >> (s_ - 1)) & 1)) continue;
        const u64 nu = (up & ~bit64(p - 1)) | bit64(r - 1), nd = (dn & ~bit64(q - 1)) | bit64(s_ - 1);
        const HkScan sc = hk_scan_body<false>(t, nu, nd, up, dn);
        if (sc.norm2 <= 0) continue;
        if (sliced) {
          u64 ru = 0, rd = 0; int k = 1;
#pragma nounroll
          for (u64 d = sc.ru; d; d &= d - 1, k++) ru += binom[ctz64(d) * SQ_BINOM_STRIDE + k];
          k = 1;
#pragma nounroll
          for (u64 d = sc.rd; d; d &= d - 1, k++) rd += binom[ctz64(d) * SQ_BINOM_STRIDE + k];
          const u64 kk = ru * n_dn_strings + rd;
          if (!(kk >= key_lo && kk < key_hi)) continue;
        }
        if (ou) { ou[cnt] = sc.ru; od[cnt] = sc.rd; onum[cnt] = sc.phase_w_rep * sqrt((double)sc.norm2) * permutation_factor(up, nu) * permutation_factor(dn, nd); }
        cnt++;
      }
    }
  }
  return cnt;
}
__device__ __noinline__ void hci_fill_hubbardk_sym(const ChemTab &t, u64 up, u64 dn, double c, double den, double *onum, double *oden, u64 cnt) {
  const int n2i = hk_scan_body<false>(t, up, dn, up, dn).norm2;
  const double norm_i = sqrt((double)n2i);
#pragma nounroll
  for (u64 k = 0; k < cnt; k++) { onum[k] = (n2i > 0) ? (t.hk_ubyn * (onum[k] / norm_i)) * c : 0.0; oden[k] = den; }      // (a source without a state in the sector: elements 0, as hamiltonian_hubbard_k_space_sym has them)
}
// hubbard2 (find_connected_dets_hubbard, hubbard.f90:5306-5457): sites ascending, at each site the up electron before the dn electron, for each
// electron the four directions in hub_nbr's order (LEFT, RIGHT, UP, DOWN) -- the "generation order" of diag_mode 2; a hop exists when the
// neighbour is allowed and empty in that spin's string.  The reference puts the source last; here it is slot 0, as for every system.  At most
// 4 nelec hops, no two to the same child (the set-up refuses a periodic direction of length 2).  Every |H| is |t|, so the screen |H c| > eps
// (strict, on the product) keeps all of a source's hops or none, and the caller makes it.  Two out-of-line calls as for hubbardk:
// hci_gen_hubbard counts the hops and, given ou / od, writes the children (a slice selects on the child's det_key; the counting pass and the
// writing pass make the same decisions); hci_fill_hubbard then writes h_hubbard's own value for the pair times c, and e_mix_den.
__device__ __noinline__ u64 hci_gen_hubbard(const ChemTab &t, const u64 *binom, u64 n_dn_strings, u64 up, u64 dn, u64 *ou, u64 *od, u64 key_lo, u64 key_hi) {
  const bool sliced = !(key_lo == 0 && key_hi == ~0ull);
  u64 cnt = 0;
#pragma nounroll
  for (u64 e = up | dn; e; e &= e - 1) {
    const int site = ctz64(e) + 1;
#pragma nounroll
    for (int sp = 0; sp < 2; sp++) {
      const u64 cfg = sp ? dn : up;
      if (!((cfg >> (site - 1)) & 1)) continue;
#pragma nounroll
      for (int k = 0; k < 4; k++) {
        const int nb = t.hub_nbr[site][k];
        if (!nb || ((cfg >> (nb - 1)) & 1)) continue;
        const u64 nc = (cfg & ~bit64(site - 1)) | bit64(nb - 1);
        const u64 nu = sp ? up : nc, nd = sp ? nc : dn;
        if (sliced) {                     // det_key, one electron at a time, as hci_gen_hubbardk
          u64 ru = 0, rd = 0; int j = 1;
#pragma nounroll
          for (u64 d = nu; d; d &= d - 1, j++) ru += binom[ctz64(d) * SQ_BINOM_STRIDE + j];
          j = 1;
#pragma nounroll
          for (u64 d = nd; d; d &= d - 1, j++) rd += binom[ctz64(d) * SQ_BINOM_STRIDE + j];
          const u64 kk = ru * n_dn_strings + rd;
          if (!(kk >= key_lo && kk < key_hi)) continue;
        }
        if (ou) { ou[cnt] = nu; od[cnt] = nd; }      // null in the counting pass
        cnt++;
      }
    }
  }
  return cnt;
}
__device__ __noinline__ void hci_fill_hubbard(const ChemTab &t, u64 up, u64 dn, double c, double den, const u64 *ou, const u64 *od, double *onum, double *oden, u64 cnt) {
#pragma nounroll
  for (u64 k = 0; k < cnt; k++) { onum[k] = h_hubbard(t, up, dn, ou[k], od[k]) * c; oden[k] = den; }
}
template <bool REC>
__global__ void __launch_bounds__(TPB) k_hci_gen(ChemDev dev, const u64 *__restrict__ rup, const u64 *__restrict__ rdn, const double *__restrict__ coef,
                                                 double eps_var, int diag_mode, long long n_ref, int pass, u64 *__restrict__ counts,
                                                 const u64 *__restrict__ offs, u64 *__restrict__ ou, u64 *__restrict__ od,
                                                 double *__restrict__ onum, double *__restrict__ oden, u64 key_lo, u64 key_hi, ActiveSpace as,
                                                 double *__restrict__ orec_old, unsigned *__restrict__ orec_pk) {
  __shared__ ChemTab t;
  __shared__ unsigned char s_lut[HEG_LUT_MAX];        // plane wave (kx,ky,kz) -> orbital id, 0 = not in the basis (find_orb_id, heg.f90:752-771)
  stage_tab(&t, dev.tab, dev.tab_words);
  if (t.sys_type == 1) {
    const int W = 2 * t.heg_nmax + 1;
    for (int k = threadIdx.x; k < W * W * W; k += TPB) s_lut[k] = 0;
    __syncthreads();
    for (int o = 1 + threadIdx.x; o <= t.norb; o += TPB)
      s_lut[((t.krel[o][0] + t.heg_nmax) * W + (t.krel[o][1] + t.heg_nmax)) * W + (t.krel[o][2] + t.heg_nmax)] = (unsigned char)o;
    __syncthreads();
  }
  long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= n_ref) return;
  const double c = coef[i];
  if (c == 0.0) { if (!pass) counts[i] = 0; return; }
  const double eps = eps_var / fabs(c);
  const u64 up = rup[i], dn = rdn[i];
  const int n = t.norb;
  const double sqrt2 = sqrt(2.0), sqrt2inv = 1.0 / sqrt2;
  u64 cnt = 0; const u64 base = pass ? offs[i] : 0;
  // diag_mode 2 ("raw", for the semistochastic PT): e_mix_den carries the index of the reference determinant instead
  // [key_lo, key_hi): only connections whose determinant key falls in this slice are kept -- the PT stage
  // of a large space is done in slices of the connected space, each with exact sums (the role of
  // n_energy_batch, hci.f90:642); the full range keeps everything without computing keys
  const bool sliced = !(key_lo == 0 && key_hi == ~0ull);
  double hii = 0.0;
  if constexpr (REC) { if (pass) hii = h_any(t, dev.integrals, up, dn, up, dn); }
#define EMIT(U, D, M, DEN, PK) do { bool in_ = true; if (sliced) { const u64 kk_ = det_key(dev, (U), (D)); in_ = (kk_ >= key_lo && kk_ < key_hi); } \
    if (in_) { if (pass) { ou[base + cnt] = (U); od[base + cnt] = (D); onum[base + cnt] = (M) * c; oden[base + cnt] = (diag_mode == 2) ? (double)i : (DEN); \
      if constexpr (REC) { orec_old[base + cnt] = hii; orec_pk[base + cnt] = (PK); } } cnt++; } } while (0)
  { double hd = (diag_mode == 1) ? ((t.sys_type == 3) ? h_hubbardk(t, up, dn, up, dn) : h_any(t, dev.integrals, up, dn, up, dn)) : 0.0;      // (hubbardk: the plain diagonal also with space_sym, see hci_gen_hubbardk_sym)
    EMIT(up, dn, hd, c, DU_NONE); }
  if (t.sys_type == 1) {
    // find_important_connected_dets_heg, heg.f90:2475-2727: no single excitations (momentum); every
    // double p,q -> r,s with k_p + k_q = k_r + k_s whose |H| exceeds eps/|c|.  The reference walks
    // |H|-sorted translation-invariant lists and stops at absH <= eps (:2608, :2629); here each
    // candidate's element is evaluated and screened -- the same set, 91 pairs x norb holes for 14
    // electrons.  Same-spin pairs take r < s (:2618).
    const int nm = t.heg_nmax, W = 2 * nm + 1;
    for (int cls = 0; cls < 3; cls++) {
      const u64 A = (cls == 1) ? dn : up, B = (cls == 0) ? up : dn;     // strings of the first / second electron
      for (u64 ea = A; ea; ea &= ea - 1) {
        const int pa = ctz64(ea) + 1;
        for (u64 eb = (cls == 2) ? B : (ea & (ea - 1)); eb; eb &= eb - 1) {
          const int qb = ctz64(eb) + 1;
          const int sx = t.krel[pa][0] + t.krel[qb][0], sy = t.krel[pa][1] + t.krel[qb][1], sz = t.krel[pa][2] + t.krel[qb][2];
          for (u64 hr = t.orb_mask & ~A; hr; hr &= hr - 1) {
            const int r = ctz64(hr) + 1;
            const int kx = sx - t.krel[r][0], ky = sy - t.krel[r][1], kz = sz - t.krel[r][2];
            if (kx < -nm || kx > nm || ky < -nm || ky > nm || kz < -nm || kz > nm) continue;
            const int s_ = s_lut[((kx + nm) * W + (ky + nm)) * W + (kz + nm)];
            if (!s_) continue;
            if (cls != 2 && s_ <= r) continue;
            if ((B >> (s_ - 1)) & 1) continue;
            u64 nu = up, nd = dn;
            if (cls == 0) nu = (up & ~bit64(pa - 1) & ~bit64(qb - 1)) | bit64(r - 1) | bit64(s_ - 1);
            else if (cls == 1) nd = (dn & ~bit64(pa - 1) & ~bit64(qb - 1)) | bit64(r - 1) | bit64(s_ - 1);
            else { nu = (up & ~bit64(pa - 1)) | bit64(r - 1); nd = (dn & ~bit64(qb - 1)) | bit64(s_ - 1); }
            const double mel = h_heg(t, up, dn, nu, nd);
            if (!(fabs(mel) > eps)) continue;
            EMIT(nu, nd, mel, 0.0, du_pack(pa + (cls == 1 ? n : 0), qb + (cls == 0 ? 0 : n), r + (cls == 1 ? n : 0), s_ + (cls == 0 ? 0 : n)));
          }
        }
      }
    }
    if (!pass) counts[i] = cnt;
    return;
  }
  if (t.sys_type == 2) {
    if (t.hub_t != 0.0 && fabs(t.hub_t * c) > eps_var) {      // |H c| > eps, with the one |H| there is; t == 0: no hops at all
      const u64 at = base + cnt;
      const u64 m = hci_gen_hubbard(t, dev.binom, dev.n_dn_strings, up, dn, pass ? ou + at : nullptr, pass ? od + at : nullptr, key_lo, key_hi);
      if (pass) hci_fill_hubbard(t, up, dn, c, (diag_mode == 2) ? (double)i : 0.0, ou + at, od + at, onum + at, oden + at, m);
      cnt += m;
    }
    if (!pass) counts[i] = cnt;
    return;
  }
  if (t.sys_type == 3) {
    if (fabs(t.hk_ubyn * c) > eps_var) {      // |H c| > eps, with the one |H| there is
      const u64 at = base + cnt;
      if (t.hk_sym) {
        const u64 m = hci_gen_hubbardk_sym(t, dev.binom, dev.n_dn_strings, up, dn, pass ? ou + at : nullptr, pass ? od + at : nullptr, pass ? onum + at : nullptr, key_lo, key_hi);
        if (pass) hci_fill_hubbardk_sym(t, up, dn, c, (diag_mode == 2) ? (double)i : 0.0, onum + at, oden + at, m);
        cnt += m;
      } else {
        const u64 m = hci_gen_hubbardk(t, dev.binom, dev.n_dn_strings, up, dn, pass ? ou + at : nullptr, pass ? od + at : nullptr, key_lo, key_hi);
        if (pass) hci_fill_hubbardk(t, up, dn, c, (diag_mode == 2) ? (double)i : 0.0, ou + at, od + at, onum + at, oden + at, m);
        cnt += m;
      }
    }
    if (!pass) counts[i] = cnt;
    return;
  }
  // singles
  for (int sp = 0; sp < 2; sp++) {
    const u64 occ = sp ? dn : up;
    for (u64 e = occ; e; e &= e - 1) {
      const int pe = ctz64(e) + 1;
      for (u64 h = t.sym_mask[t.orbsym[pe]] & ~occ; h; h &= h - 1) {
        const int r = ctz64(h) + 1;
        u64 nu = up, nd = dn;
        if (!sp) nu = (up & ~bit64(pe - 1)) | bit64(r - 1); else nd = (dn & ~bit64(pe - 1)) | bit64(r - 1);
        if (active_space_skip(as, nu, nd)) continue;
        if (t.time_sym) { if (nu == nd && t.z < 0) continue; if (up == nd && dn == nu) continue; }
        double mel = h_single(t, dev.integrals, up, dn, nu, nd);
        if (fabs(mel) < eps) continue;
        if (t.time_sym) {
          if (up == dn && nu != nd) mel = sqrt2inv * mel;
          if (nu == nd && up != dn) mel = sqrt2 * mel;
          if (nu > nd) { u64 x = nu; nu = nd; nd = x; mel = t.z * mel; }
        }
        EMIT(nu, nd, mel, 0.0, DU_NONE);
      }
    }
  }
  if (!(eps > dev.max_double)) {
    // occupied pairs: up-up, dn-dn, up-dn (chemistry.f90:7000-7021)
    for (int cls = 0; cls < 3; cls++) {
      const u64 A = (cls == 1) ? dn : up, B = (cls == 0) ? up : dn;
      for (u64 ea = A; ea; ea &= ea - 1) {
        const int pa = ctz64(ea) + 1;
        for (u64 eb = (cls == 2) ? B : (ea & (ea - 1)); eb; eb &= eb - 1) {
          const int qb = ctz64(eb) + 1;
          int p = pa + (cls == 1 ? n : 0), q = qb + (cls == 0 ? 0 : n);
          int p2 = p, q2 = q;
          const bool both_dn = (cls == 1), swapped = (cls == 2 && p > q - n);
          if (both_dn) { p2 = p - n; q2 = q - n; }
          if (swapped) { p2 = q - n; q2 = p + n; }
          const long long e = (p2 > q2) ? ((long long)p2 * (p2 - 1)) / 2 + q2 : ((long long)q2 * (q2 - 1)) / 2 + p2;
          const long long k0 = dev.pq_ind[e] - 1; const int kc = dev.pq_count[e];
          for (int hh = 0; hh < kc; hh++) {
            if (dev.hb_absH[k0 + hh] <= eps) break;
            int r = dev.hb_r[k0 + hh], s = dev.hb_s[k0 + hh];
            if (both_dn) { r += n; s += n; }
            if (swapped) { int rt = s - n; s = r + n; r = rt; }
            if (r <= n ? ((up >> (r - 1)) & 1) : ((dn >> (r - n - 1)) & 1)) continue;
            if (s <= n ? ((up >> (s - 1)) & 1) : ((dn >> (s - n - 1)) & 1)) continue;
            u64 nu = up, nd = dn;
            if (p <= n) nu &= ~bit64(p - 1); else nd &= ~bit64(p - n - 1);
            if (q <= n) nu &= ~bit64(q - 1); else nd &= ~bit64(q - n - 1);
            if (r <= n) nu |= bit64(r - 1); else nd |= bit64(r - n - 1);
            if (s <= n) nu |= bit64(s - 1); else nd |= bit64(s - n - 1);
            if (active_space_skip(as, nu, nd)) continue;
            if (t.time_sym) { if (nu == nd && t.z < 0) continue; if (up == nd && dn == nu) continue; }
            double mel = 0.0;
            if (pass) {
              mel = h_double(t, dev.integrals, up, dn, nu, nd);
              if (t.time_sym) {
                if (up == dn && nu != nd) mel = sqrt2inv * mel;
                if (nu == nd && up != dn) mel = sqrt2 * mel;
              }
            }
            if (t.time_sym && nu > nd) { u64 x = nu; nu = nd; nd = x; mel = t.z * mel; }
            EMIT(nu, nd, mel, 0.0, du_pack(p, q, r, s));
          }
        }
      }
    }
  }
#undef EMIT
  if (!pass) counts[i] = cnt;
}
// dedup of the sorted connection list: sums e_mix_num / e_mix_den of equal determinants
// left to right (merge_original_with_spawned3, tools.f90:577-660).
// REC: the merged determinant keeps the record of the FIRST entry of its run in the sorted order (the sort is stable: the first in
// generation order).  The reference keeps whichever its merge leaves; every record of a run leads to the same H_aa up to rounding,
// so no parity with the reference's choice is claimed.
__global__ void __launch_bounds__(TPB) k_hci_heads(const u64 *__restrict__ skey, u64 *__restrict__ flags, long long n) {
  long long j = (long long)blockIdx.x * TPB + threadIdx.x;
  if (j < n) flags[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1ull : 0ull;
}
template <bool REC>
__global__ void __launch_bounds__(TPB) k_hci_dedup(const u64 *__restrict__ skey, const u32 *__restrict__ perm, const u64 *__restrict__ flags,
                                                   const u64 *__restrict__ pos, const u64 *__restrict__ iu, const u64 *__restrict__ id,
                                                   const double *__restrict__ inum, const double *__restrict__ iden,
                                                   u64 *__restrict__ ou, u64 *__restrict__ od, double *__restrict__ onum, double *__restrict__ oden, long long n,
                                                   const double *__restrict__ irec_old, const unsigned *__restrict__ irec_pk,
                                                   double *__restrict__ orec_old, unsigned *__restrict__ orec_pk) {
  long long j = (long long)blockIdx.x * TPB + threadIdx.x;
  if (j >= n || !flags[j]) return;
  const u64 key = skey[j]; u32 t = perm[j];
  double a = inum[t], b = iden[t];
  for (long long jj = j + 1; jj < n && skey[jj] == key; jj++) { a = a + inum[perm[jj]]; b = b + iden[perm[jj]]; }
  const u64 o = pos[j];
  ou[o] = iu[t]; od[o] = id[t]; onum[o] = a; oden[o] = b;
  if constexpr (REC) { orec_old[o] = irec_old[t]; orec_pk[o] = irec_pk[t]; }
}

// ================================================================ semistochastic PT2 (second_order_pt_alias, hci.f90:1314-1660)
// the sampled determinants of one sample, gathered from the plan's resident variational list: the generator's input
__global__ void __launch_bounds__(TPB) k_pt2s_gather(const int *__restrict__ ids, const u64 *__restrict__ vu, const u64 *__restrict__ vd,
                                                     const double *__restrict__ vc, u64 *__restrict__ ru, u64 *__restrict__ rd, double *__restrict__ rc, long long n) {
  long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i < n) { const int s = ids[i]; ru[i] = vu[s]; rd[i] = vd[s]; rc[i] = vc[s]; }
}
// The weighted segmented sums of one sample and its finish in one pass over the sorted raw connections (hci.f90:1452-1640).
// The thread that lands on the head of a run of equal keys owns the connected determinant k: it drops k if k is in the variational
// space (binary search on the sorted ranks, as k_pt2_terms; this drops every source's own slot too), walks the run left to right --
// the stable sort keeps generation order, so the additions have one fixed order -- forming from x = H_ki c_i and the source's
// w/p (src: the raw mode's index of the source among the sampled determinants)
//     term1 = sum x w/p                     term2 = sum x^2 ((n_mc-1) w/p - (w/p)^2)
// and the same two over the connections with |x| > eps_pt_big, then H_kk and the term
//     (term1^2 + term2 - term1_big^2 - term2_big) / (E_var - H_kk).
// Runs are short (k is reached from a handful of the <= n_mc sources), hence one thread per run as k_hci_dedup; no head flags,
// scan or compaction: nothing is copied out.  Grid-stride, one partial sum and one count per block (fixed tree, no atomics).
__global__ void __launch_bounds__(TPB) k_pt2s_terms(ChemDev dev, const u64 *__restrict__ skey, const u32 *__restrict__ perm, const u64 *__restrict__ cu,
                                                    const u64 *__restrict__ cd, const double *__restrict__ x, const double *__restrict__ src,
                                                    const double *__restrict__ wop, long long n, const u64 *__restrict__ vkeys, long long nv, double e_var,
                                                    double eps_big, double n_mc_m1, double *__restrict__ partial, u64 *__restrict__ pcount) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  double acc = 0.0; u64 cnt = 0;
  for (long long j = (long long)blockIdx.x * TPB + threadIdx.x; j < n; j += (long long)gridDim.x * TPB) {
    const u64 key = skey[j];
    if (j > 0 && skey[j - 1] == key) continue;         // not a head
    long long lo = 0, hi = nv;                         // first variational rank >= key
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (vkeys[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo < nv && vkeys[lo] == key) continue;         // inside the variational space
    const u32 p0 = perm[j];
    double t1 = 0.0, t2 = 0.0, t1b = 0.0, t2b = 0.0;
    for (long long jj = j; jj < n && skey[jj] == key; jj++) {
      const u32 p = (jj == j) ? p0 : perm[jj];
      const double xv = x[p], w = wop[(int)src[p]];
      const double a1 = xv * w, a2 = (xv * xv) * (n_mc_m1 * w - w * w);
      const bool big = fabs(xv) > eps_big;
      if (jj == j) { t1 = a1; t2 = a2; t1b = big ? a1 : 0.0; t2b = big ? a2 : 0.0; }
      else { t1 = t1 + a1; t2 = t2 + a2; t1b = t1b + (big ? a1 : 0.0); t2b = t2b + (big ? a2 : 0.0); }
    }
    const u64 u = cu[p0], d = cd[p0];
    const double hkk = h_any(t, dev.integrals, u, d, u, d);
    acc += (t1 * t1 + t2 - t1b * t1b - t2b) / (e_var - hkk);
    cnt++;
  }
  __shared__ double red[TPB / 64]; __shared__ u64 redc[TPB / 64];
  for (int o = 32; o > 0; o >>= 1) { acc += __shfl_down(acc, o, 64); cnt += __shfl_down(cnt, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; redc[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0; u64 k = 0;
    for (int q = 0; q < TPB / 64; q++) { v += red[q]; k += redc[q]; }
    partial[blockIdx.x] = v; pcount[blockIdx.x] = k;
  }
}
// the block partials of k_pt2s_terms in block order: lane l of one wavefront adds its contiguous share left to right, then the
// fixed shuffle tree; out[0] = the sum (a double), out[1] = the count -- the 16 bytes a sample sends back
__global__ void __launch_bounds__(64) k_pt2s_final(const double *__restrict__ partial, const u64 *__restrict__ pcount, int nb, u64 *__restrict__ out) {
  const int chunk = (nb + 63) / 64, lane = threadIdx.x;
  double a = 0.0; u64 k = 0;
  for (int q = lane * chunk; q < (lane + 1) * chunk && q < nb; q++) { a += partial[q]; k += pcount[q]; }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); k += __shfl_down(k, o, 64); }
  if (lane == 0) { out[0] = (u64)__double_as_longlong(a); out[1] = k; }
}
