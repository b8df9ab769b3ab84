// tdm_kernels.h -- one- and two-body transition density matrices of two coefficient vectors, bra and ket, over one determinant list
// (no counterpart in the reference, which stops at get_1rdm).  Textually included by tdm_device.hip, a translation unit and code
// object of their own (behind chem_device.h: det_key and the layout of the binomial table; and rdm2_plan.h: Rdm2Shape); the doors in
// sqmc_gpu.hip (abi_tdm.inc) launch them through tdm_launch.h, and the 2-RDM's emit, sort and column starts through rdm2_launch.h.
// Not a standalone header.
//
//   T_aa[p,q,r,s] = <bra| a+_{p up} a+_{q up} a_{s up} a_{r up} |ket>,  T_bb the same with dn,
//   T_ab[p,q,r,s] = <bra| a+_{p up} a+_{q dn} a_{s dn} a_{r up} |ket>,  flat index p + norb (q + norb (r + norb s))
// Through the intermediates of rdm2_kernels.h: T[a, b] = sum_K u_K[a] w_K[b], u the signed bra coefficients and w the signed ket
// coefficients of the same records.
//
//   k_tdm2_bra      the second value column.  rdm2's k_rdm2_emit runs on ket and writes keys, pairs and w; the parity of a record
//                   depends on its local pair alone, so this kernel recomputes it from l = t % R and writes u = +-bra beside it
//   k_tdm2_sorted   k_rdm2_sorted with both value columns
//   k_tdm2_gram     the owner scheme of k_rdm2_gram (one owner per pair of column ranks i <= j, columns longest first, the owner
//                   strides over the shorter column in K order and bisects the longer one, block or wavefront by RDM2_HEAVY, the same
//                   tree) with two accumulators for the one search: T[A,B] += u[lo] w[t], T[B,A] += u[t] w[lo]; i == j: u[t] w[t].
//                   Entry e writes gram[2 e] = T[A,B] and gram[2 e + 1] = T[B,A] (the same number twice when i == j).  With bra == ket
//                   both are the bits of k_rdm2_gram's entry: the same products in the same order.  Swapping bra and ket swaps the two
//   k_tdm2_expand   into the zeroed dense block: (A, B) from the first accumulator and (B, A) from the second, for aa / bb the four
//                   signed images of each; an image of sign -1 is 0.0 - g, so that nothing is ever -0.0
//
// One-body, tdm[p + norb r] = <bra| a+_r a_p |ket> summed over spin = sum_sigma sum_i sign ket_i bra_k, k = determinant i with the
// sigma electron moved p -> r: the owner-computes layout of k_rdm_terms (rdm_kernels.h).  A block owns one (p <= r, sigma) and one
// chunk of TDM1_CHUNK determinants of the list in rank order; for p < r one search serves both entries,
//   tdm[p,r] += sign ket_i bra_k,   tdm[r,p] += sign bra_i ket_k
// (the second is the term of the move r -> p from k, met at its partner).  The block adds by the tree of rdm_block_store and
// k_tdm1_sum adds the chunks in chunk order, up before dn.  With bra == ket both are the bits of the 1-RDM's entry (p, r), p < r.

#include "rdm2_index.h"      // rdm2_entry, rdm2_put

// u[t] of record t = determinant t / R, local pair t % R: the parity of k_rdm2_emit
__global__ void __launch_bounds__(TPB) k_tdm2_bra(const double *__restrict__ sc, long long n, Rdm2Shape sh, double *__restrict__ U) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  if (t >= n * sh.R) return;
  const long long j = t / sh.R; const int l = (int)(t - j * sh.R);
  int par;
  if (sh.kind == RDM2_AB) {
    const int x = l / sh.ndn, y = l - x * sh.ndn;
    par = x + y;
  } else {
    int y = 1; while ((y + 1) * y / 2 <= l) y++;      // l = y (y - 1) / 2 + x, x < y
    const int x = l - y * (y - 1) / 2;
    par = x + y - 1;
  }
  const double c = sc[j];
  U[t] = (par & 1) ? 0.0 - c : c;
}
__global__ void __launch_bounds__(TPB) k_tdm2_sorted(const u32 *__restrict__ perm, const u64 *__restrict__ K, const u32 *__restrict__ P, const double *__restrict__ U,
                                                     const double *__restrict__ W, long long nrec, u64 *__restrict__ sK, u32 *__restrict__ sP,
                                                     double *__restrict__ sU, double *__restrict__ sW) {
  const long long k = (long long)blockIdx.x * TPB + threadIdx.x;
  if (k >= nrec) return;
  const u32 r = perm[k];
  sK[k] = K[r]; sP[k] = P[r]; sU[k] = U[r]; sW[k] = W[r];
}
// G = 256: a block per entry; G = 64: a wavefront per entry, four to a block.  Entries [e0, e1); gram: two doubles per entry
template <int G>
__global__ void __launch_bounds__(256) k_tdm2_gram(const u64 *__restrict__ sK, const double *__restrict__ sU, const double *__restrict__ sW, const u32 *__restrict__ start,
                                                   const u32 *__restrict__ col, long long e0, long long e1, double *__restrict__ gram) {
  __shared__ double red[2][4];
  const int lane = G == 256 ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  const long long e = e0 + (G == 256 ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + (threadIdx.x >> 6));
  double ab = 0.0, ba = 0.0;
  bool diag = false;
  if (e < e1) {                                        // the same for every lane of a wavefront (of the block when G = 256)
    long long i, j; rdm2_entry(e, &i, &j);
    diag = i == j;
    const u32 A = col[i], B = col[j];                  // column A is at least as long as column B
    const long long a0 = start[A], a1 = start[A + 1], b0 = start[B], b1 = start[B + 1];
    for (long long t = b0 + lane; t < b1; t += G) {
      const double ut = sU[t], wt = sW[t];
      if (diag) { ab += ut * wt; continue; }
      const u64 key = sK[t];
      long long lo = a0, hi = a1;                      // first K of column A >= key
      while (lo < hi) { const long long mid = (lo + hi) >> 1; if (sK[mid] < key) lo = mid + 1; else hi = mid; }
      if (lo < a1 && sK[lo] == key) { ab += sU[lo] * wt; ba += ut * sW[lo]; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { ab += __shfl_down(ab, o, 64); ba += __shfl_down(ba, o, 64); }
  if (G == 256) {
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ab; red[1][threadIdx.x >> 6] = ba; }
    __syncthreads();
    if (threadIdx.x == 0 && e < e1) {
      const double x = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      gram[2 * e] = x; gram[2 * e + 1] = diag ? x : (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
  } else if (lane == 0 && e < e1) { gram[2 * e] = ab; gram[2 * e + 1] = diag ? ab : ba; }
}
// one thread per entry of the Gram matrix; out: norb^4 doubles, zeroed
__global__ void __launch_bounds__(TPB) k_tdm2_expand(const double *__restrict__ gram, const u32 *__restrict__ col, long long nent, int kind, int norb, double *__restrict__ out) {
  const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
  if (e >= nent) return;
  long long i, j; rdm2_entry(e, &i, &j);
  const int A = (int)col[i], B = (int)col[j];
  const double g = gram[2 * e], h = gram[2 * e + 1], mg = 0.0 - g, mh = 0.0 - h;
  if (kind == RDM2_AB) {
    const int p = A % norb, q = A / norb, r = B % norb, s = B / norb;
    rdm2_put(out, norb, p, q, r, s, g); rdm2_put(out, norb, r, s, p, q, h);
    return;
  }
  int q = (int)((1.0 + sqrt(1.0 + 8.0 * (double)A)) * 0.5); while (q > 1 && q * (q - 1) / 2 > A) q--; while ((q + 1) * q / 2 <= A) q++;
  int s = (int)((1.0 + sqrt(1.0 + 8.0 * (double)B)) * 0.5); while (s > 1 && s * (s - 1) / 2 > B) s--; while ((s + 1) * s / 2 <= B) s++;
  const int p = A - q * (q - 1) / 2, r = B - s * (s - 1) / 2;      // p < q, r < s
  rdm2_put(out, norb, p, q, r, s, g); rdm2_put(out, norb, q, p, r, s, mg); rdm2_put(out, norb, p, q, s, r, mg); rdm2_put(out, norb, q, p, s, r, g);
  rdm2_put(out, norb, r, s, p, q, h); rdm2_put(out, norb, r, s, q, p, mh); rdm2_put(out, norb, s, r, p, q, mh); rdm2_put(out, norb, s, r, q, p, h);
}

// (-1)^(bits of s strictly between positions p and r), p < r: rdm_sign of rdm_kernels.h
__device__ __forceinline__ double tdm1_sign(u64 s, int p, int r) {
  const u64 between = maskr64(r) & ~maskr64(p + 1);
  return (popc64(s & between) & 1) ? -1.0 : 1.0;
}
// grid (chunks, norb (norb + 1) / 2, 2): blockIdx.y = r (r + 1) / 2 + p with p <= r, blockIdx.z = sigma.  skey: the list's sorted
// ranks; sym: norb labels or null.  partial[((chunk * npr + y) * 2 + sigma) * 2 + {0: (p, r), 1: (r, p)}]
__global__ void __launch_bounds__(TDM1_T) k_tdm1_terms(ChemDev dev, const u64 *__restrict__ su, const u64 *__restrict__ sd, const double *__restrict__ sb, const double *__restrict__ sk,
                                                       long long n, const u64 *__restrict__ skey, int norb, const unsigned char *__restrict__ sym, double *__restrict__ partial) {
  __shared__ double red[2][TDM1_T / 64];
  const int sigma = blockIdx.z;
  int r = 0; while ((r + 1) * (r + 2) / 2 <= (int)blockIdx.y) r++;
  const int p = (int)blockIdx.y - r * (r + 1) / 2;
  double *out = partial + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 + sigma) * 2;
  if (sym && sym[p] != sym[r]) { if (threadIdx.x == 0) { out[0] = 0.0; out[1] = 0.0; } return; }      // the same for every thread of the block
  const long long j0 = (long long)blockIdx.x * TDM1_CHUNK, j1 = (j0 + TDM1_CHUNK < n) ? j0 + TDM1_CHUNK : n;
  const u64 bp = bit64(p), br = bit64(r);
  double pr = 0.0, rp = 0.0;
  for (long long j = j0 + threadIdx.x; j < j1; j += TDM1_T) {
    const u64 u = su[j], d = sd[j], s = sigma ? d : u;
    if (!(s & bp)) continue;
    if (p == r) { pr += sk[j] * sb[j]; continue; }
    if (s & br) continue;
    const u64 s2 = (s ^ bp) | br;
    const u64 key = sigma ? det_key(dev, u, s2) : det_key(dev, s2, d);
    long long lo = 0, hi = n;                          // first rank >= key
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (skey[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo >= n || skey[lo] != key) continue;
    const double sg = tdm1_sign(s, p, r);
    pr += sg * sk[j] * sb[lo]; rp += sg * sb[j] * sk[lo];
  }
  for (int o = 32; o > 0; o >>= 1) { pr += __shfl_down(pr, o, 64); rp += __shfl_down(rp, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = pr; red[1][threadIdx.x >> 6] = rp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < TDM1_T / 64; q++) { a += red[0][q]; b += red[1][q]; }
    out[0] = a; out[1] = p == r ? a : b;
  }
}
// one thread per (p, r): chunks in chunk order, up then dn.  flat index of the output: p + norb r
__global__ void __launch_bounds__(TPB) k_tdm1_sum(const double *__restrict__ partial, int nchunks, int norb, double *__restrict__ tdm) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= norb * norb) return;
  const int p = e % norb, r = e / norb, lo = p < r ? p : r, hi = p < r ? r : p;
  const size_t npr = (size_t)norb * (norb + 1) / 2, stride = npr * 4, at = ((size_t)hi * (hi + 1) / 2 + lo) * 4 + (p > r ? 1 : 0);
  double a = 0.0, b = 0.0;
  for (int q = 0; q < nchunks; q++) a += partial[q * stride + at];
  for (int q = 0; q < nchunks; q++) b += partial[q * stride + at + 2];
  tdm[e] = a + b;
}
