// rdm2_kernels.h -- two-body reduced density matrix of an HCI wavefunction, three spin blocks (no counterpart in the reference,
// which stops at get_1rdm).  Textually included by rdm2_device.hip, a translation unit and code object of their own (behind chem_device.h:
// colex_rank and the layout of the binomial table); the door in sqmc_gpu.hip launches them through rdm2_launch.h and sorts with
// scan_sort.h.  Not a standalone header.
//
//   G_aa[p,q,r,s] = <a+_{p up} a+_{q up} a_{s up} a_{r up}>,  G_bb the same with dn,  G_ab[p,q,r,s] = <a+_{p up} a+_{q dn} a_{s dn} a_{r up}>
// 0-based, flat index p + norb (q + norb (r + norb s)), determinants = all up operators in front of all dn operators.
//
// Through the (N-2)-electron intermediates: G[a, b] = sum_K v_K[a] v_K[b], v_K[(r, s)] = c_i sign(a_s a_r on i), K = i - r - s, with
// a, b orbital pairs (r < s for aa / bb, every (r, s) for ab).  A (K, pair) names one determinant, so a record is one signed
// coefficient.  sign = (-1)^(electrons of the string below r, + those below s other than r); for ab the dn operator also passes the
// nup - 1 up electrons, a factor common to v_K[a] and v_K[b] that is left out.
//
//   k_rdm2_emit     every determinant writes its C(nup,2) / C(ndn,2) / nup ndn records at fixed offsets (no count, no scan): the
//                   key of K (colex ranks of its two strings at the reduced electron counts), the pair index, the value
//   sort            by (pair, K).  One radix sort of the word (pair << kbits | K) when pair index and K fit 64 bits together
//                   (every chem system of up to ~40 orbitals); otherwise two stable sorts, K first and the pair index second.
//                   A column (the records of one pair) then holds strictly increasing K
//   k_rdm2_sorted   the records in sorted order;  k_rdm2_colstart  the columns' offsets by bisection
//   k_rdm2_gram     one owner per entry (a <= b) of the non-empty columns, columns ranked longest first by the host: the owner
//                   strides over the shorter column in K order and bisects the longer one; each lane adds its products in K order,
//                   the lanes add through the fixed shuffle tree (and, for a block, the wavefronts left to right).  An entry whose
//                   shorter column has RDM2_HEAVY records or more is owned by a 256-thread block, every other one by a wavefront:
//                   the entries in flat order run from the most work to the least, so the long ones start first and the many short
//                   ones fill in behind them.  Which lane meets which record depends on the columns alone: an entry has the same
//                   bits run to run, for any order of the caller's list and whichever other blocks the call asked for.  No
//                   floating-point atomics, no matrix cores.
//   k_rdm2_expand   into the zeroed dense block: (a, b) and (b, a), and for aa / bb the four signed images of p < q, r < s; an image
//                   of sign -1 is 0.0 - g, so that nothing is ever -0.0.  G[p,q,r,s] == G[r,s,p,q] and the antisymmetries hold exactly.

#include "rdm2_index.h"      // rdm2_entry, rdm2_put: shared with tdm_kernels.h

__device__ __forceinline__ int rdm2_nth_bit(u64 s, int k) { for (int q = 0; q < k; q++) s &= s - 1; return ctz64(s); }

// record t = determinant t / R, local pair t % R.  sortkey: the word (oneword) or the key of K; idx: the record's own index
__global__ void __launch_bounds__(TPB) k_rdm2_emit(const u64 *__restrict__ binom, const u64 *__restrict__ su, const u64 *__restrict__ sd, const double *__restrict__ sc,
                                                   long long n, Rdm2Shape sh, u64 *__restrict__ sortkey, u32 *__restrict__ idx, u64 *__restrict__ K,
                                                   u32 *__restrict__ P, double *__restrict__ V) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  if (t >= n * sh.R) return;
  const long long j = t / sh.R; const int l = (int)(t - j * sh.R);
  const u64 u = su[j], d = sd[j];
  u64 ku = u, kd = d; int par; u32 pair;
  if (sh.kind == RDM2_AB) {
    const int x = l / sh.ndn, y = l - x * sh.ndn;
    const int r = rdm2_nth_bit(u, x), s = rdm2_nth_bit(d, y);
    ku = u ^ bit64(r); kd = d ^ bit64(s); par = x + y; pair = (u32)(r + sh.norb * s);
  } else {
    const u64 str = sh.kind == RDM2_BB ? d : u;
    int y = 1; while ((y + 1) * y / 2 <= l) y++;      // l = y (y - 1) / 2 + x, x < y
    const int x = l - y * (y - 1) / 2;
    const int r = rdm2_nth_bit(str, x), s = rdm2_nth_bit(str, y);
    const u64 k2 = str ^ bit64(r) ^ bit64(s);
    if (sh.kind == RDM2_BB) kd = k2; else ku = k2;
    par = x + y - 1; pair = (u32)(s * (s - 1) / 2 + r);
  }
  const u64 key = colex_rank(binom, ku) * sh.n_dn_k + colex_rank(binom, kd);
  const double c = sc[j];
  sortkey[t] = sh.oneword ? (((u64)pair << sh.kbits) | key) : key;
  idx[t] = (u32)t; K[t] = key; P[t] = pair; V[t] = (par & 1) ? 0.0 - c : c;
}
// second pass of the two-pass order: the pair index of the records in K order
__global__ void __launch_bounds__(TPB) k_rdm2_pairkeys(const u32 *__restrict__ perm, const u32 *__restrict__ P, long long nrec, u64 *__restrict__ key2) {
  const long long k = (long long)blockIdx.x * TPB + threadIdx.x;
  if (k < nrec) key2[k] = P[perm[k]];
}
__global__ void __launch_bounds__(TPB) k_rdm2_sorted(const u32 *__restrict__ perm, const u64 *__restrict__ K, const u32 *__restrict__ P, const double *__restrict__ V, long long nrec,
                                                     u64 *__restrict__ sK, u32 *__restrict__ sP, double *__restrict__ sV) {
  const long long k = (long long)blockIdx.x * TPB + threadIdx.x;
  if (k >= nrec) return;
  const u32 r = perm[k];
  sK[k] = K[r]; sP[k] = P[r]; sV[k] = V[r];
}
// start[p] = first sorted record of pair index >= p, p = 0 .. npairs
__global__ void __launch_bounds__(TPB) k_rdm2_colstart(const u32 *__restrict__ sP, long long nrec, int npairs, u32 *__restrict__ start) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p > npairs) return;
  long long lo = 0, hi = nrec;
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (sP[mid] < (u32)p) lo = mid + 1; else hi = mid; }
  start[p] = (u32)lo;
}
// G = 256: a block per entry; G = 64: a wavefront per entry, four to a block.  Entries [e0, e1)
template <int G>
__global__ void __launch_bounds__(256) k_rdm2_gram(const u64 *__restrict__ sK, const double *__restrict__ sV, const u32 *__restrict__ start, const u32 *__restrict__ col,
                                                   long long e0, long long e1, double *__restrict__ gram) {
  __shared__ double red[4];
  const int lane = G == 256 ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const long long e = e0 + (G == 256 ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + (threadIdx.x >> 6));
  double acc = 0.0;
  if (e < e1) {                                        // the same for every lane of a wavefront (of the block when G = 256)
    long long i, j; rdm2_entry(e, &i, &j);
    const u32 A = col[i], B = col[j];                  // column A is at least as long as column B
    const long long a0 = start[A], a1 = start[A + 1], b0 = start[B], b1 = start[B + 1];
    for (long long t = b0 + lane; t < b1; t += G) {
      const double v = sV[t];
      if (i == j) { acc += v * v; continue; }
      const u64 key = sK[t];
      long long lo = a0, hi = a1;                      // first K of column A >= key
      while (lo < hi) { const long long mid = (lo + hi) >> 1; if (sK[mid] < key) lo = mid + 1; else hi = mid; }
      if (lo < a1 && sK[lo] == key) acc += v * sV[lo];
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if (G == 256) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && e < e1) gram[e] = (red[0] + red[1]) + (red[2] + red[3]);
  } else if (lane == 0 && e < e1) gram[e] = acc;
}
// one thread per entry of the Gram matrix; out: norb^4 doubles, zeroed
__global__ void __launch_bounds__(TPB) k_rdm2_expand(const double *__restrict__ gram, const u32 *__restrict__ col, long long nent, int kind, int norb, double *__restrict__ out) {
  const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
  if (e >= nent) return;
  long long i, j; rdm2_entry(e, &i, &j);
  const int A = (int)col[i], B = (int)col[j];
  const double g = gram[e], m = 0.0 - g;
  if (kind == RDM2_AB) {
    const int p = A % norb, q = A / norb, r = B % norb, s = B / norb;
    rdm2_put(out, norb, p, q, r, s, g); rdm2_put(out, norb, r, s, p, q, g);
    return;
  }
  int q = (int)((1.0 + sqrt(1.0 + 8.0 * (double)A)) * 0.5); while (q > 1 && q * (q - 1) / 2 > A) q--; while ((q + 1) * q / 2 <= A) q++;
  int s = (int)((1.0 + sqrt(1.0 + 8.0 * (double)B)) * 0.5); while (s > 1 && s * (s - 1) / 2 > B) s--; while ((s + 1) * s / 2 <= B) s++;
  const int p = A - q * (q - 1) / 2, r = B - s * (s - 1) / 2;      // p < q, r < s
  rdm2_put(out, norb, p, q, r, s, g); rdm2_put(out, norb, q, p, r, s, m); rdm2_put(out, norb, p, q, s, r, m); rdm2_put(out, norb, q, p, s, r, g);
  rdm2_put(out, norb, r, s, p, q, g); rdm2_put(out, norb, r, s, q, p, m); rdm2_put(out, norb, s, r, p, q, m); rdm2_put(out, norb, s, r, q, p, g);
}
