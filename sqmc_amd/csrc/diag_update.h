// diag_update.h -- H_aa of a determinant one double excitation away from a determinant whose H_ii is known, in O(n_elec):
// get_new_diag_elem (chemistry.f90:9649-9739) and get_new_diag_elem_heg (heg.f90:3357-3453).  Textually included by sqmc_gpu.hip.
//
// The record (diag_elem_info, common_run): old_diag_elem = H_ii of the source and the excitation p, q -> r, s in the reference's
// spin-orbital numbering (1..norb up, norb+1..2 norb dn), r of p's spin and s of q's (find_important_connected_dets_chem fills it
// at chemistry.f90:7148-7152).  From it
//   H_aa = H_ii + h(r) + h(s) - h(p) - h(q)                                      one-body        (:9697)
//               + direct(r,s) - direct(p,q)                                      O(1) direct     (:9700)
//               - exchange(r,s) + exchange(p,q)            if p, q of one spin   O(1) exchange   (:9703-9705)
//               + sum_i direct(i,r) + direct(i,s) - direct(i,p) - direct(i,q)    i occupied in the NEW determinant, up then dn,
//                                                                                 r and s skipped (:9710-9719)
//               + sum_i - exchange(i,r) + exchange(i,p)  [i of p's spin]  - exchange(i,s) + exchange(i,q)  [i of q's spin]   (:9722-9737)
// Two forms.  du_lane: one lane, every addition in the reference's statement order -- bit for bit what a left-to-right evaluation
// of those statements gives.  du_rounds: the 16 lanes of a group take one occupied orbital each, add their own terms and the
// group adds the 16 partial sums in a butterfly; the O(1) part is as in du_lane.  Same terms, another order of additions.
//
// Single excitations and a source's own slot: the reference's record holds old_diag_elem = 1e51 for them (chemistry.f90:6898,
// 6990) and find_doubly_excited recomputes such a determinant from scratch ("compute the easy way for now", semistoch.f90:2185-2186).
// So does this library: their packed record is 0 and the caller falls back to h_any.
//
// Electron gas: the reference has the routine but does not call it (semistoch.f90:2190-2193 recomputes, "this cost is negligible"),
// and as written its one-body part vanishes -- heg.f90's integral_value returns 0 for p == q (:3465) before it looks for the
// one-body case (:3470) -- so it would lose the kinetic energy.  Here the same statements run with the integrals the HEG
// Hamiltonian has (hamiltonian_heg, heg.f90:845-1011): h(i) = |k_i|^2 / 2, direct = 0 (the uniform background cancels it),
// exchange(i,j) = 4 pi / (|k_i - k_j|^2 L^3) as integral_value forms it (:3482-3483).
#pragma once

#define DU_NONE 0u                       // packed record of a connection that has none (single excitation, self slot): from scratch
__device__ __forceinline__ unsigned du_pack(int p, int q, int r, int s) { return (unsigned)p | ((unsigned)q << 8) | ((unsigned)r << 16) | ((unsigned)s << 24); }   // 2 norb <= 128

struct DuChem {                          // integral_value of chemistry.f90 on the packed table
  const ChemTab &t; const double *__restrict__ ints;
  __device__ __forceinline__ double one(int i) const { return ints[integral_index(t, i, i, t.norb + 1, t.norb + 1)]; }
  __device__ __forceinline__ double dir(int i, int j) const { return ints[integral_index(t, i, i, j, j)]; }
  __device__ __forceinline__ double exc(int i, int j) const { return ints[integral_index(t, i, j, j, i)]; }
};
struct DuHeg {
  const ChemTab &t;
  __device__ __forceinline__ double one(int i) const { return heg_sumsq(t, t.kvec[i]) * 0.5; }
  __device__ __forceinline__ double dir(int, int) const { return 0.0; }
  __device__ __forceinline__ double exc(int i, int j) const {
    const double FOUR_PI = 4.0 * (4.0 * atan(1.0)), L = t.length_cell;
    double s = 0.0;
    for (int k = 0; k < t.n_dim; k++) { const double d = t.kvec[j][k] - t.kvec[i][k]; s = s + d * d; }
    return FOUR_PI / (s * (L * L * L));
  }
};

struct DuRec { int p, q, r, s; bool p_up, q_up; u64 skip_up, skip_dn; };      // p..s spatial (1..norb)
__device__ __forceinline__ DuRec du_unpack(int norb, unsigned pk) {
  const int p_in = pk & 255u, q_in = (pk >> 8) & 255u, r_in = (pk >> 16) & 255u, s_in = pk >> 24;
  DuRec e;
  e.p_up = p_in <= norb; e.q_up = q_in <= norb;
  e.p = e.p_up ? p_in : p_in - norb; e.q = e.q_up ? q_in : q_in - norb;
  e.r = r_in > norb ? r_in - norb : r_in; e.s = s_in > norb ? s_in - norb : s_in;
  // "if (i==r_in.or.i==s_in) cycle" in the up loops, "i==r_in-norb.or.i==s_in-norb" in the dn loops
  e.skip_up = (r_in <= norb ? bit64(r_in - 1) : 0ull) | (s_in <= norb ? bit64(s_in - 1) : 0ull);
  e.skip_dn = (r_in > norb ? bit64(r_in - norb - 1) : 0ull) | (s_in > norb ? bit64(s_in - norb - 1) : 0ull);
  return e;
}
// A record is usable when every table index it leads to is inside the tables and it describes a double excitation that ends in
// (new_up, new_dn): orbitals in 1..2 norb, p != q, r != s, r of p's spin and s of q's, r and s occupied in the new determinant,
// p and q empty in it (they are the two orbitals the source had and the new determinant has not), electron numbers right.
__device__ __forceinline__ bool du_record_ok(const ChemTab &t, int p, int q, int r, int s, u64 nu, u64 nd) {
  const int n = t.norb, n2 = 2 * t.norb;
  if (p < 1 || p > n2 || q < 1 || q > n2 || r < 1 || r > n2 || s < 1 || s > n2) return false;
  if (p == q || r == s) return false;
  if ((p <= n) != (r <= n) || (q <= n) != (s <= n)) return false;
  if ((nu & ~t.orb_mask) || (nd & ~t.orb_mask) || popc64(nu) != t.nup || popc64(nd) != t.ndn) return false;
  const auto occ = [&](int o) { return o <= n ? ((nu >> (o - 1)) & 1ull) : ((nd >> (o - n - 1)) & 1ull); };
  return occ(r) && occ(s) && !occ(p) && !occ(q);
}

template <class IV>
__device__ __forceinline__ double du_head(const IV &iv, const DuRec &e, double old_diag) {
  double v = old_diag + iv.one(e.r) + iv.one(e.s) - iv.one(e.p) - iv.one(e.q);
  v = v + iv.dir(e.r, e.s) - iv.dir(e.p, e.q);
  if (e.p_up == e.q_up) v = v - iv.exc(e.r, e.s) + iv.exc(e.p, e.q);
  return v;
}
// ---- one lane, the reference's order
template <class IV>
__device__ inline double du_lane(const IV &iv, int norb, double old_diag, unsigned pk, u64 nu, u64 nd) {
  const DuRec e = du_unpack(norb, pk);
  double v = du_head(iv, e, old_diag);
  for (u64 b = nu & ~e.skip_up; b; b &= b - 1) { const int i = ctz64(b) + 1; v = v + iv.dir(i, e.r) + iv.dir(i, e.s) - iv.dir(i, e.p) - iv.dir(i, e.q); }
  for (u64 b = nd & ~e.skip_dn; b; b &= b - 1) { const int i = ctz64(b) + 1; v = v + iv.dir(i, e.r) + iv.dir(i, e.s) - iv.dir(i, e.p) - iv.dir(i, e.q); }
  if (e.p_up || e.q_up)
    for (u64 b = nu & ~e.skip_up; b; b &= b - 1) {
      const int i = ctz64(b) + 1;
      if (e.p_up) v = v - iv.exc(i, e.r) + iv.exc(i, e.p);
      if (e.q_up) v = v - iv.exc(i, e.s) + iv.exc(i, e.q);
    }
  if (!e.p_up || !e.q_up)
    for (u64 b = nd & ~e.skip_dn; b; b &= b - 1) {
      const int i = ctz64(b) + 1;
      if (!e.p_up) v = v - iv.exc(i, e.r) + iv.exc(i, e.p);
      if (!e.q_up) v = v - iv.exc(i, e.s) + iv.exc(i, e.q);
    }
  return v;
}
// ---- 16 lanes: every lane of a group owns one record; in round w the group works on the record of its lane w.  Lane g takes the
// occupied orbitals number g, g + 16, ... of the new determinant (up ascending, then dn, r and s left out), adds their direct and
// exchange terms, the butterfly adds the 16 partial sums (every lane ends with the same bits), the O(1) part comes first as in
// du_lane.  have: this lane's record is to be evaluated; all 64 lanes of the wavefront must make the call.
#define DU_GROUP 16
template <class IV>
__device__ inline double du_rounds(const IV &iv, int norb, bool have, double old_diag, unsigned pk, u64 nu, u64 nd) {
  const int g = threadIdx.x & (DU_GROUP - 1);
  double mine = 0.0;
  for (int w = 0; w < DU_GROUP; w++) {
    if (!__shfl((int)have, w, DU_GROUP)) continue;                  // the same decision in all 16 lanes
    const double old_w = __shfl(old_diag, w, DU_GROUP);
    const unsigned pk_w = (unsigned)__shfl((int)pk, w, DU_GROUP);
    const u64 nu_w = __shfl(nu, w, DU_GROUP), nd_w = __shfl(nd, w, DU_GROUP);
    const DuRec e = du_unpack(norb, pk_w);
    const u64 bu = nu_w & ~e.skip_up, bd = nd_w & ~e.skip_dn;
    const int cu = popc64(bu), ntot = cu + popc64(bd);
    double part = 0.0;
    for (int k = g; k < ntot; k += DU_GROUP) {
      const bool is_up = k < cu;
      const int i = bk_nth_orb(is_up ? bu : bd, is_up ? k : k - cu) + 1;
      double c = iv.dir(i, e.r) + iv.dir(i, e.s) - iv.dir(i, e.p) - iv.dir(i, e.q);
      if (e.p_up == is_up) c = c - iv.exc(i, e.r) + iv.exc(i, e.p);
      if (e.q_up == is_up) c = c - iv.exc(i, e.s) + iv.exc(i, e.q);
      part = part + c;
    }
    for (int o = DU_GROUP / 2; o > 0; o >>= 1) part = part + __shfl_xor(part, o, DU_GROUP);
    const double v = du_head(iv, e, old_w) + part;
    if (g == w) mine = v;
  }
  return mine;
}

// H_aa of one connected determinant from its record; FORM 0 = du_lane, 1 = du_rounds (then every lane of the wavefront calls it,
// need or not).  A connection without a record (DU_NONE) is computed from scratch, as the reference does for single excitations.
template <int FORM>
__device__ __forceinline__ double du_haa(const ChemTab &t, const double *__restrict__ ints, bool need, u64 u, u64 d, double old_diag, unsigned pk) {
  const bool upd = need && pk != DU_NONE;
  double v = 0.0;
  if (need && !upd) v = h_any(t, ints, u, d, u, d);
  if (FORM == 0) {
    if (upd) v = (t.sys_type == 1) ? du_lane(DuHeg{t}, t.norb, old_diag, pk, u, d) : du_lane(DuChem{t, ints}, t.norb, old_diag, pk, u, d);
  } else {
    const double w = (t.sys_type == 1) ? du_rounds(DuHeg{t}, t.norb, upd, old_diag, pk, u, d) : du_rounds(DuChem{t, ints}, t.norb, upd, old_diag, pk, u, d);
    if (upd) v = w;
  }
  return v;
}

// ---- the batch door's kernel: validate, then evaluate; a bad record raises the flag and is never evaluated
template <int FORM>
__global__ void __launch_bounds__(TPB) k_diag_update_batch(ChemDev dev, const double *__restrict__ old_diag, const int *__restrict__ pqrs, const u64 *__restrict__ nu,
                                                           const u64 *__restrict__ nd, double *__restrict__ out, long long n, int *__restrict__ bad) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  bool ok = false; double od = 0.0; unsigned pk = DU_NONE; u64 u = 0, d = 0;
  if (i < n) {
    const int p = pqrs[4 * i], q = pqrs[4 * i + 1], r = pqrs[4 * i + 2], s = pqrs[4 * i + 3];
    u = nu[i]; d = nd[i]; od = old_diag[i];
    ok = du_record_ok(t, p, q, r, s, u, d);
    if (ok) pk = du_pack(p, q, r, s); else *bad = 1;
  }
  const double v = du_haa<FORM>(t, dev.integrals, ok, u, d, od, pk);
  if (i < n) out[i] = v;
}

// ---- second_order_pt's sum with H_aa from the record (k_pt2_terms, door_kernels.h, is the from-scratch form and stays as it is):
// the same membership search, the same owner of every term, the same block tree
__device__ __forceinline__ double du_block_sum(double acc) {
  __shared__ double red[TPB / 64];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  double v = 0.0;
  if (threadIdx.x == 0) for (int q = 0; q < TPB / 64; q++) v += red[q];
  return v;
}
template <int FORM>
__global__ void __launch_bounds__(TPB) k_pt2_terms_upd(ChemDev dev, const u64 *__restrict__ cu, const u64 *__restrict__ cd, const double *__restrict__ num,
                                                       const double *__restrict__ rold, const unsigned *__restrict__ rpk, long long n,
                                                       const u64 *__restrict__ vkeys, long long nv, double e_var, double *__restrict__ partial) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  double acc = 0.0;
  for (long long base = (long long)blockIdx.x * TPB; base < n; base += (long long)gridDim.x * TPB) {      // uniform: du_rounds needs every lane
    const long long i = base + threadIdx.x;
    bool need = false; u64 u = 0, d = 0;
    if (i < n) {
      u = cu[i]; d = cd[i];
      const u64 key = det_key(dev, u, d);
      long long lo = 0, hi = nv;
      while (lo < hi) { const long long mid = (lo + hi) >> 1; if (vkeys[mid] < key) lo = mid + 1; else hi = mid; }
      need = !(lo < nv && vkeys[lo] == key);
    }
    const double haa = du_haa<FORM>(t, dev.integrals, need, u, d, need ? rold[i] : 0.0, need ? rpk[i] : DU_NONE);
    if (need) { const double x = num[i]; acc += x * x / (e_var - haa); }
  }
  const double v = du_block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}
// ---- one sample of the semistochastic PT2 with H_kk from the record of the first connection of k's run (k_pt2s_terms,
// hci_kernels.h, is the from-scratch form and stays as it is): the same heads, the same membership search, the same left-to-right
// sums inside a run, the same owner of every term and the same block tree
template <int FORM>
__global__ void __launch_bounds__(TPB) k_pt2s_terms_upd(ChemDev dev, const u64 *__restrict__ skey, const u32 *__restrict__ perm, const u64 *__restrict__ cu,
                                                        const u64 *__restrict__ cd, const double *__restrict__ x, const double *__restrict__ src,
                                                        const double *__restrict__ rold, const unsigned *__restrict__ rpk,
                                                        const double *__restrict__ wop, long long n, const u64 *__restrict__ vkeys, long long nv, double e_var,
                                                        double eps_big, double n_mc_m1, double *__restrict__ partial, u64 *__restrict__ pcount) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  double acc = 0.0; u64 cnt = 0;
  for (long long base = (long long)blockIdx.x * TPB; base < n; base += (long long)gridDim.x * TPB) {
    const long long j = base + threadIdx.x;
    bool need = false; u32 p0 = 0;
    if (j < n) {
      const u64 key = skey[j];
      if (!(j > 0 && skey[j - 1] == key)) {              // a head
        long long lo = 0, hi = nv;
        while (lo < hi) { const long long mid = (lo + hi) >> 1; if (vkeys[mid] < key) lo = mid + 1; else hi = mid; }
        need = !(lo < nv && vkeys[lo] == key);
      }
      if (need) p0 = perm[j];
    }
    double t1 = 0.0, t2 = 0.0, t1b = 0.0, t2b = 0.0;
    if (need) {
      const u64 key = skey[j];
      for (long long jj = j; jj < n && skey[jj] == key; jj++) {
        const u32 p = (jj == j) ? p0 : perm[jj];
        const double xv = x[p], w = wop[(int)src[p]];
        const double a1 = xv * w, a2 = (xv * xv) * (n_mc_m1 * w - w * w);
        const bool big = fabs(xv) > eps_big;
        if (jj == j) { t1 = a1; t2 = a2; t1b = big ? a1 : 0.0; t2b = big ? a2 : 0.0; }
        else { t1 = t1 + a1; t2 = t2 + a2; t1b = t1b + (big ? a1 : 0.0); t2b = t2b + (big ? a2 : 0.0); }
      }
    }
    const double hkk = du_haa<FORM>(t, dev.integrals, need, need ? cu[p0] : 0ull, need ? cd[p0] : 0ull, need ? rold[p0] : 0.0, need ? rpk[p0] : DU_NONE);
    if (need) { acc += (t1 * t1 + t2 - t1b * t1b - t2b) / (e_var - hkk); cnt++; }
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
