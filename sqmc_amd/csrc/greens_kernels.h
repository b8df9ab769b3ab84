// greens_kernels.h -- zeroth-order Green's function of an HCI wavefunction (get_zeroth_order_variational_greens_function,
// hci.f90:3849-4050).  Textually included by sqmc_gpu.hip (one translation unit: ChemDev, det_key, h_diag, rdm_sign); not a
// standalone header.
//
//   G0_np1(w, p, q) = sum_sigma sum_i c_i c_k / (w - (H_mm - e0)),  m = i + q sigma (q empty in i),    k = m - p sigma (p occupied in m)
//   G0_nm1(w, p, q) = sum_sigma sum_i c_i c_k / (w - (e0 - H_mm)),  m = i - q sigma (q occupied in i), k = m + p sigma (p empty in m)
// k in the list; H_mm the chem diagonal of the N+-1 electron determinant from scratch (h_diag works from the bit strings alone).  A
// term is the rounded product c_i c_k divided by the rounded denominator, as the reference forms it (:3944).  fermi = 0: no sign,
// as the reference; fermi = 1: the sign of a_p a+_q (N+1: -(-1)^between for p != q) or a+_p a_q (N-1: (-1)^between) on ordered
// strings, between = the sigma electrons strictly between p and q (rdm_sign).
//
// k_gf_poles: one thread per (determinant of a tile of the list in rank order, slot).  Slots of N+1: the empty up orbitals ascending,
// then the empty dn orbitals; of N-1: the occupied up orbitals, then the occupied dn orbitals.  It writes x = H_mm - e0 (N+1) or
// e0 - H_mm (N-1): H_mm once per (determinant, q, sigma), not once per p.
// k_gf_terms: a block owns one (p, q, sigma) and one chunk of GF_CHUNK consecutive determinants.  Thread t looks at the determinants
// t, t + GF_T, ... of the chunk: bit tests, k, its rank by binary search in the sorted ranks.  The hits (A = c_i c_k [sign], x) are
// packed into LDS in determinant order (ballots and a 16-entry prefix: no atomics, at most one hit per determinant for a fixed
// (p, q, sigma)).  After the barrier thread t takes the frequencies t, t + GF_T, ... of the frequency tile and adds A[h] / (w - x[h])
// over the hits in that order into partial[chunk][i_w][p][q][sigma].
// k_gf_sum: one thread per (i_w, p, q) adds the chunks in chunk order onto the running sums of the two spins, and with `last` writes
// g[i_w + n_w (p + norb q)] = up + dn.  A sum continues across the tiles of the list in the same sequence, so that an entry has the
// same bits however the list and the frequencies are tiled, run to run and for any order of the caller's list.
// Work memory: the poles of one list tile, partial of one (list tile, frequency tile), the running sums (2 n_w norb^2).

#define GF_T 256                 // threads of a block
#define GF_CHUNK 1024            // determinants of a block's chunk (four per thread)
#define GF_WTILE 256             // frequencies of a frequency tile

// the s-th (0-based) set bit of `bits`, as a position
__device__ __forceinline__ int gf_nth_bit(u64 bits, int s) {
  for (int k = 0; k < s; k++) bits &= bits - 1;
  return ctz64(bits);
}
// H_mm: the statements of h_diag (chem_device.h), which reads the bit strings alone (never t.nup / t.ndn) and so serves N+-1 electrons.
// Its own function: one more caller of h_diag in this translation unit stops the compiler inlining h_diag into the kernels that were
// here before (they gain a call, 16 bytes of stack and up to 22 VGPRs).
__device__ inline double gf_h_mm(const ChemTab &t, const double *__restrict__ ints, u64 up, u64 dn) {
  const int n1 = t.norb + 1;
  double e1 = 0.0;
  SQ_ORDERED_SUM4(e1, up, +, integral_index(t, j, j, n1, n1))
  if (dn == up) e1 = e1 * 2.0;
  else { SQ_ORDERED_SUM4(e1, dn, +, integral_index(t, j, j, n1, n1)) }
  double ex = 0.0, di = 0.0;
  for (u64 a = up; a; a &= a - 1) { const int i = ctz64(a) + 1; SQ_ORDERED_SUM4(ex, a & (a - 1), -, integral_index(t, i, j, j, i)) }
  if (dn == up) ex = ex * 2.0;
  else if (dn != 0)
    for (u64 a = dn; a; a &= a - 1) { const int i = ctz64(a) + 1; SQ_ORDERED_SUM4(ex, a & (a - 1), -, integral_index(t, i, j, j, i)) }
  for (u64 occ = up | dn; occ; occ &= occ - 1) {
    const int i0 = ctz64(occ), i = i0 + 1;
    if ((up >> i0) & 1) {
      SQ_ORDERED_SUM4(di, up & ~maskr64(i), +, integral_index(t, i, i, j, j))
      SQ_ORDERED_SUM4(di, dn, +, integral_index(t, i, i, j, j))
    }
    if ((dn >> i0) & 1) { SQ_ORDERED_SUM4(di, dn & ~maskr64(i), +, integral_index(t, i, i, j, j)) }
  }
  return e1 + (ex + di) + t.nuclear;
}
// j0: first determinant of the list tile; nd: determinants of the tile; n_su: slots of the up string (norb - nup or nup)
template <bool NP1>
__global__ void __launch_bounds__(TPB) k_gf_poles(ChemDev dev, const u64 *__restrict__ su, const u64 *__restrict__ sd, long long j0, long long nd, int n_su, int nslot,
                                                  double e0, double *__restrict__ poles) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
  if (idx >= nd * nslot) return;
  const long long jj = idx / nslot; const int slot = (int)(idx - jj * nslot);
  u64 u = su[j0 + jj], d = sd[j0 + jj];
  const bool dn = slot >= n_su;
  const u64 s = dn ? d : u;
  const u64 from = NP1 ? (~s & t.orb_mask) : s;
  const u64 b = bit64(gf_nth_bit(from, dn ? slot - n_su : slot));
  if (dn) d ^= b; else u ^= b;
  const double h = gf_h_mm(t, dev.integrals, u, d);
  poles[idx] = NP1 ? (h - e0) : (e0 - h);
}
// grid (chunks of the list tile, norb * norb * 2); partial[(chunk * wt + i_w) * gridDim.y + pair]
template <bool NP1>
__global__ void __launch_bounds__(GF_T) k_gf_terms(ChemDev dev, const u64 *__restrict__ su, const u64 *__restrict__ sd, const double *__restrict__ sc,
                                                   const u64 *__restrict__ skey, long long n, long long j0, long long nd, const double *__restrict__ poles,
                                                   int norb, int n_su, int nslot, int fermi, const double *__restrict__ w, int wt, double *__restrict__ partial) {
  __shared__ double hA[GF_CHUNK], hX[GF_CHUNK];
  __shared__ int cnt[GF_CHUNK / 64 + 1];
  const int pair = blockIdx.y, sigma = pair & 1, q = (pair >> 1) % norb, p = (pair >> 1) / norb;
  const long long c0 = (long long)blockIdx.x * GF_CHUNK;            // within the tile
  const u64 bp = bit64(p), bq = bit64(q);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double a_[GF_CHUNK / GF_T], x_[GF_CHUNK / GF_T]; bool hit_[GF_CHUNK / GF_T];
#pragma unroll
  for (int r = 0; r < GF_CHUNK / GF_T; r++) {
    const long long jj = c0 + r * GF_T + threadIdx.x;
    bool hit = false; double a = 0.0, x = 0.0;
    if (jj < nd) {
      const long long j = j0 + jj;
      const u64 u = su[j], d = sd[j], s = sigma ? d : u;
      // N+1: q empty in s, p occupied in s + q.  N-1: q occupied in s, p empty in s - q
      const bool q_ok = NP1 ? !(s & bq) : (s & bq) != 0;
      const bool p_ok = (p == q) || (NP1 ? (s & bp) != 0 : !(s & bp));
      if (q_ok && p_ok) {
        long long lo = j;
        if (p != q) {
          const u64 s2 = s ^ bq ^ bp;
          const u64 key = sigma ? det_key(dev, u, s2) : det_key(dev, s2, d);
          long long hi = n; lo = 0;                             // first rank >= key
          while (lo < hi) { const long long mid = (lo + hi) >> 1; if (skey[mid] < key) lo = mid + 1; else hi = mid; }
          hit = lo < n && skey[lo] == key;
        } else hit = true;
        if (hit) {
          a = sc[j] * sc[lo];
          if (fermi && p != q) a = (NP1 ? -rdm_sign(s, p, q) : rdm_sign(s, p, q)) * a;
          const int below = popc64(s & maskr64(q));
          x = poles[jj * nslot + (sigma ? n_su : 0) + (NP1 ? q - below : below)];
        }
      }
    }
    a_[r] = a; x_[r] = x; hit_[r] = hit;
    const u64 bal = __ballot(hit);
    if (lane == 0) cnt[r * (GF_T / 64) + wave] = popc64(bal);
  }
  __syncthreads();
  int nh = 0;
#pragma unroll
  for (int r = 0; r < GF_CHUNK / GF_T; r++) {
    int base = 0;
    for (int k = 0; k < r * (GF_T / 64) + wave; k++) base += cnt[k];
    const u64 bal = __ballot(hit_[r]);
    if (hit_[r]) { const int at = base + popc64(bal & maskr64(lane)); hA[at] = a_[r]; hX[at] = x_[r]; }
  }
  for (int k = 0; k < GF_CHUNK / 64; k++) nh += cnt[k];
  __syncthreads();
  for (int iw = threadIdx.x; iw < wt; iw += GF_T) {
    const double ww = w[iw];
    double acc = 0.0;
    for (int h = 0; h < nh; h++) acc += hA[h] / (ww - hX[h]);
    partial[((size_t)blockIdx.x * wt + iw) * gridDim.y + pair] = acc;
  }
}
// one thread per (i_w of the tile, e = p norb + q): run[((w0 + i_w) norb^2 + e) 2 + sigma] += the chunks in chunk order; last: g = up + dn
__global__ void __launch_bounds__(TPB) k_gf_sum(const double *__restrict__ partial, int nchunks, int norb, int wt, int w0, int n_w, int last,
                                                double *__restrict__ run, double *__restrict__ g) {
  const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
  const int nn = norb * norb;
  if (idx >= (long long)wt * nn) return;
  const int iw = (int)(idx / nn), e = (int)(idx - (long long)iw * nn);
  const size_t stride = (size_t)wt * nn * 2, at = (size_t)iw * nn * 2 + 2 * e;
  double *r = run + ((size_t)(w0 + iw) * nn + e) * 2;
  double a = r[0], b = r[1];
  for (int c = 0; c < nchunks; c++) a += partial[c * stride + at];
  for (int c = 0; c < nchunks; c++) b += partial[c * stride + at + 1];
  r[0] = a; r[1] = b;
  if (last) g[(size_t)(w0 + iw) + (size_t)n_w * ((e / norb) + (size_t)norb * (e % norb))] = a + b;
}
