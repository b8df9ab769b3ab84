// orbopt_kernels.h -- the generalised Fock matrix, the orbital gradient and the diagonal orbital Hessian from the density matrices of
// a chem context.  Compiled by orbopt_device.hip alone (a code object of its own), launched through orbopt_launch.h.
//
//   F[a,P]     = sum_r h[a,r] D[P,r] + sum_qrs (ar|qs) G[P,q,r,s]
//   grad[p,q]  = 2 (F[p,q] - F[q,p])
//   Y[xP,yQ]   = 2 h[x,y] D[P,Q] + 2 sum_rs { (xy|rs) G[P,r,Q,s] + (xr|ys) (G[P,Q,r,s] + G[P,s,r,Q]) }
//   hdiag[p,q] = -2 (F[p,p] + F[q,q]) + Y[pq,pq] + Y[qp,qp] - 2 Y[pq,qp],   hdiag[p,p] = 0
//
// Orbitals 0-based.  Every norb x norb array has the flat index (first + norb second), G the index p + norb (q + norb (r + norb s)).
// The integrals are the context's packed table; pair[a norb + r] = combine_2(a + 1, r + 1) is uploaded by the door, which has checked
// that it is symmetric, one-to-one and inside the table, so every index formed here lies inside it.  h[a,r] = ints[hbase + pair[a,r]],
// hbase = A (A - 1) / 2 with A = combine_2(norb + 1, norb + 1).
//
// The Fock GEMM runs over K = (q, r, s), k = q + norb (r + norb s): for fixed k, G[., k] is a contiguous run of norb doubles and
// (a r|q s) over a is a gather.  Block b owns the chunks [b cpb, (b + 1) cpb) of ORB_KC triples each and writes one partial tile
// part[b][a + norb P]; k_orb_fock_reduce adds the one-body term and the partials.  Vector FMAs, no MFMA and no atomics.  The order of
// additions of an entry F[a,P] is:  t_b = fma chain over the k of block b, ascending, from 0.0;
//                                   F = (fma chain over r of h[a,r] D[P,r], ascending, from 0.0) + t_0 + t_1 + ... in ascending b.
// fma is explicit (the library is compiled with -ffp-contract=off).  No sum starts from or can end in -0.0: every chain starts at +0.0.

__device__ __forceinline__ int orb_tri(int a, int b) { return (a > b) ? (a * (a - 1)) / 2 + b : (b * (b - 1)) / 2 + a; }
// (q, r, s) of k + step from those of k
__device__ __forceinline__ void orb_advance(int &q, int &r, int &s, int n, int step) {
  q += step;
  while (q >= n) { q -= n; if (++r == n) { r = 0; ++s; } }
}

// grid: plan.nblocks blocks of ORB_T threads; dynamic LDS: norb^2 ints (the pair table)
template <int TM>
__global__ void __launch_bounds__(ORB_T) k_orb_fock_part(const double *__restrict__ ints, const int *__restrict__ pair, const double *__restrict__ G,
                                                          int n, long long K, long long nchunks, long long cpb, double *__restrict__ part) {
  constexpr int NT = 16 * TM, KSTEP = ORB_T / NT, NJ = ORB_KC / KSTEP;
  __shared__ double As[ORB_KC][NT], Bs[ORB_KC][NT];
  extern __shared__ int orb_pair[];
  const int tid = threadIdx.x, nn = n * n;
  for (int e = tid; e < nn; e += ORB_T) orb_pair[e] = pair[e];
  const long long c0 = (long long)blockIdx.x * cpb, c1 = (c0 + cpb < nchunks) ? c0 + cpb : nchunks;
  // staging: this thread loads row li of the triples kk0 + j KSTEP of a chunk
  const int li = tid % NT, kk0 = tid / NT;
  long long kfirst = c0 * ORB_KC + kk0;
  int q = (int)(kfirst % n), r = (int)((kfirst / n) % n), s = (int)(kfirst / ((long long)n * n));      // s may be >= n past the end: never used there
  // compute: rows a = tx TM + i, columns P = ty TM + j
  const int tx = tid & 15, ty = tid >> 4;
  double acc[TM][TM];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = 0.0;
  __syncthreads();
  for (long long c = c0; c < c1; c++) {
    const long long k0 = c * ORB_KC;
    int qq = q, rr = r, ss = s;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int kk = kk0 + j * KSTEP;
      const long long k = k0 + kk;
      double av = 0.0, bv = 0.0;
      if (k < K && li < n) {
        av = ints[orb_tri(orb_pair[rr * n + li], orb_pair[qq * n + ss])];      // (li rr|qq ss): the pair table is symmetric
        bv = G[(size_t)k * n + li];
      }
      As[kk][li] = av; Bs[kk][li] = bv;
      orb_advance(qq, rr, ss, n, KSTEP);
    }
    orb_advance(q, r, s, n, ORB_KC);
    __syncthreads();
    const int kmax = (K - k0 < ORB_KC) ? (int)(K - k0) : ORB_KC;
    for (int kk = 0; kk < kmax; kk++) {
      double x[TM], y[TM];
#pragma unroll
      for (int i = 0; i < TM; i++) { x[i] = As[kk][tx * TM + i]; y[i] = Bs[kk][ty * TM + i]; }
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TM; j++) acc[i][j] = fma(x[i], y[j], acc[i][j]);
    }
    __syncthreads();
  }
  double *out = part + (size_t)blockIdx.x * nn;
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) {
      const int a = tx * TM + i, P = ty * TM + j;
      if (a < n && P < n) out[a + n * P] = acc[i][j];
    }
}

// one thread per entry: the one-body term, then the partial tiles in ascending block order
__global__ void __launch_bounds__(ORB_T) k_orb_fock_reduce(const double *__restrict__ ints, const int *__restrict__ pair, int hbase, const double *__restrict__ D,
                                                            const double *__restrict__ part, int n, long long nblocks, double *__restrict__ F) {
  const int nn = n * n, e = blockIdx.x * ORB_T + threadIdx.x;
  if (e >= nn) return;
  const int a = e % n, P = e / n;
  double acc = 0.0;
  for (int r = 0; r < n; r++) acc = fma(ints[hbase + pair[a * n + r]], D[P + n * r], acc);
  for (long long b = 0; b < nblocks; b++) acc += part[(size_t)b * nn + e];
  F[e] = acc;
}

// grad[p,q] = 2 (F[p,q] - F[q,p]): the two roundings are each other's negatives, so grad[p,q] == -grad[q,p]; x - x = +0.0
__global__ void __launch_bounds__(ORB_T) k_orb_grad(const double *__restrict__ F, int n, double *__restrict__ grad) {
  const int nn = n * n, e = blockIdx.x * ORB_T + threadIdx.x;
  if (e >= nn) return;
  const int p = e % n, q = e / n;
  grad[e] = (p == q) ? 0.0 : 2.0 * (F[p + n * q] - F[q + n * p]);
}

// grid: norb^2 blocks of ORB_HD_T threads, block e owns hdiag[p,q], p = e % norb, q = e / norb.  Thread t adds the terms of
// rs = t, t + ORB_HD_T, ... (r = rs % norb, s = rs / norb) in ascending order from 0.0, per rs in the order
//   Y[pq,pq]: (pp|rs) G[q,r,q,s], (pr|ps) (G[q,q,r,s] + G[q,s,r,q]);  Y[qp,qp]: the same with p and q exchanged;
//   -2 Y[pq,qp]: -2 (pq|rs) G[q,r,p,s], -2 (pr|qs) (G[q,p,r,s] + G[q,s,r,p]);
// thread 0 adds the ORB_HD_T sums in ascending t, then the three one-body products, doubles, and subtracts 2 (F[p,p] + F[q,q]).
__global__ void __launch_bounds__(ORB_HD_T) k_orb_hdiag(const double *__restrict__ ints, const int *__restrict__ pair, int hbase, const double *__restrict__ D,
                                                         const double *__restrict__ G, const double *__restrict__ F, int n, double *__restrict__ hd) {
  __shared__ double sums[ORB_HD_T];
  const int nn = n * n, e = blockIdx.x, p = e % n, q = e / n, t = threadIdx.x;
  if (p == q) { if (t == 0) hd[e] = 0.0; return; }
  const size_t N = (size_t)n;
#define ORB_G4(a, b, c, d) G[(size_t)(a) + N * ((size_t)(b) + N * ((size_t)(c) + N * (size_t)(d)))]
#define ORB_I4(a, b, c, d) ints[orb_tri(pair[(a) * n + (b)], pair[(c) * n + (d)])]
  double acc = 0.0;
  for (int rs = t; rs < nn; rs += ORB_HD_T) {
    const int r = rs % n, s = rs / n;
    acc = fma(ORB_I4(p, p, r, s), ORB_G4(q, r, q, s), acc);
    acc = fma(ORB_I4(p, r, p, s), ORB_G4(q, q, r, s) + ORB_G4(q, s, r, q), acc);
    acc = fma(ORB_I4(q, q, r, s), ORB_G4(p, r, p, s), acc);
    acc = fma(ORB_I4(q, r, q, s), ORB_G4(p, p, r, s) + ORB_G4(p, s, r, p), acc);
    acc = fma(-2.0 * ORB_I4(p, q, r, s), ORB_G4(q, r, p, s), acc);
    acc = fma(-2.0 * ORB_I4(p, r, q, s), ORB_G4(q, p, r, s) + ORB_G4(q, s, r, p), acc);
  }
#undef ORB_G4
#undef ORB_I4
  sums[t] = acc;
  __syncthreads();
  if (t != 0) return;
  double tot = 0.0;
  for (int k = 0; k < ORB_HD_T; k++) tot += sums[k];
  double one = fma(ints[hbase + pair[p * n + p]], D[q + n * q], 0.0);
  one = fma(ints[hbase + pair[q * n + q]], D[p + n * p], one);
  one = fma(-2.0 * ints[hbase + pair[p * n + q]], D[q + n * p], one);
  hd[e] = (2.0 * (tot + one) - 2.0 * (F[p + n * p] + F[q + n * q])) + 0.0;
}
