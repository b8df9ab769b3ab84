// orbopt_kernels.h -- the generalised Fock matrix, the orbital gradient and the diagonal orbital Hessian from the density matrices of
// a chem context; behind them the one-index transformation of the integrals and the kernel that makes an orbital Hessian-vector
// product of it (stated where they begin).  Compiled by orbopt_device.hip alone (a code object of its own), launched through orbopt_launch.h.
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

// ------------------------------------------------------------------------------------------------- the one-index transformation
//   h~[P,Q]  = sum_a kap[a,P] h[a,Q] + sum_b kap[b,Q] h[P,b]
//   (PQ|RS)~ = sum_a kap[a,P] (aQ|RS) + sum_b kap[b,Q] (Pb|RS) + sum_c kap[c,R] (PQ|cS) + sum_d kap[d,S] (PQ|Rd)
// kap[a n + P] = kappa[a,P], any real matrix.  The result has the 8-fold symmetry of the integrals and goes into their packed layout.
// The kernels number the npair = n (n + 1) / 2 pairs themselves, tri(p, q) = p (p + 1) / 2 + q for p >= q; pidx[tri(p, q)] = pair[p n + q]
// addresses the tables.  Half pass, block rs:  work[tri(P, Q) npair + rs] = first two terms, with M_rs[p][q] = (pq|rs) and kappa in LDS
// (2 n^2 doubles).  The last two terms are the first two with the pairs exchanged, so the symmetrising pass stores
// work[PQ npair + RS] + work[RS npair + PQ] for RS <= PQ.  The one-body block is the half pass on M = h, stored where it belongs.
// An entry of the half pass is (fma chain over a, ascending, from 0.0) + (fma chain over b, ascending, from 0.0); every entry has one
// owner, no atomics.  M is symmetric, so both chains read their two factors along rows: Z[i][j] = sum_k X[k][i] Y[k][j].

// acc[i][j] = sum_k X[k n + i0 + i] Y[k n + j0 + j], k ascending from 0.0; rows and columns beyond n read the last one (never stored)
template <int TM>
__device__ __forceinline__ void orb_xty(const double *__restrict__ X, const double *__restrict__ Y, int n, int i0, int j0, double (&acc)[TM][TM]) {
  int ci[TM], cj[TM];
#pragma unroll
  for (int i = 0; i < TM; i++) { ci[i] = (i0 + i < n) ? i0 + i : n - 1; cj[i] = (j0 + i < n) ? j0 + i : n - 1; }
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = 0.0;
  for (int k = 0; k < n; k++) {
    double x[TM], y[TM];
#pragma unroll
    for (int i = 0; i < TM; i++) { x[i] = X[k * n + ci[i]]; y[i] = Y[k * n + cj[i]]; }
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TM; j++) acc[i][j] = fma(x[i], y[j], acc[i][j]);
  }
}

// grid: npair blocks (ONE = false: block rs writes column rs of work) or one block (ONE = true: the one-body block into dst = the
// output table); ORB_T threads; dynamic LDS 2 n^2 doubles
template <int TM, bool ONE>
__global__ void __launch_bounds__(ORB_T) k_orb_oneidx_half(const double *__restrict__ ints, const int *__restrict__ pair, const int *__restrict__ pidx, int hbase,
                                                            const double *__restrict__ kap, int n, double *__restrict__ dst) {
  extern __shared__ double orb_lds[];
  const int nn = n * n, blk = blockIdx.x;
  const size_t npair = (size_t)n * (n + 1) / 2;
  double *Kp = orb_lds, *M = orb_lds + nn;
  const int prs = ONE ? 0 : pidx[blk];
  for (int e = threadIdx.x; e < nn; e += ORB_T) {
    Kp[e] = kap[e];
    M[e] = ONE ? ints[hbase + pair[e]] : ints[orb_tri(pair[e], prs)];
  }
  __syncthreads();
  const int nt = (n + TM - 1) / TM;
  for (int tile = threadIdx.x; tile < nt * nt; tile += ORB_T) {
    const int i0 = (tile / nt) * TM, j0 = (tile % nt) * TM;
    if (j0 > i0) continue;                                  // no entry P >= Q in the tile
    double c1[TM][TM], c2[TM][TM];
    orb_xty<TM>(Kp, M, n, i0, j0, c1);                      // sum_a kap[a,P] M[a][Q]
    orb_xty<TM>(M, Kp, n, i0, j0, c2);                      // sum_b M[b][P] kap[b,Q]
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TM; j++) {
        const int P = i0 + i, Q = j0 + j;
        if (P >= n || Q > P) continue;
        const double v = c1[i][j] + c2[i][j];
        if (ONE) dst[hbase + pair[P * n + Q]] = v;
        else dst[(size_t)(P * (P + 1) / 2 + Q) * npair + blk] = v;
      }
  }
}

// grid: ntile (ntile + 1) / 2 blocks, ntile = ceil(npair / ORB_SYM_TILE), block b owns the tile (ti, tj), tj <= ti; ORB_T threads as
// ORB_SYM_TILE columns x (ORB_T / ORB_SYM_TILE) rows.  The transposed tile goes through LDS (padded by one column), so that both
// reads of work run along its rows.
__global__ void __launch_bounds__(ORB_T) k_orb_oneidx_sym(const double *__restrict__ work, const int *__restrict__ pidx, int npair, double *__restrict__ out) {
  constexpr int TS = ORB_SYM_TILE, ROWS = ORB_T / TS;
  __shared__ double Bt[TS][TS + 1];
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ti++;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  const int x = threadIdx.x % TS, y0 = threadIdx.x / TS;
  for (int y = y0; y < TS; y += ROWS) {                     // Bt[y][x] = work[(tj TS + y) npair + ti TS + x]
    const int row = tj * TS + y, col = ti * TS + x;
    Bt[y][x] = (row < npair && col < npair) ? work[(size_t)row * npair + col] : 0.0;
  }
  __syncthreads();
  for (int y = y0; y < TS; y += ROWS) {
    const int PQ = ti * TS + y, RS = tj * TS + x;
    if (PQ >= npair || RS > PQ) continue;
    out[orb_tri(pidx[PQ], pidx[RS])] = work[(size_t)PQ * npair + RS] + Bt[x][y];
  }
}

// sigma[p,q] = gt[p,q] + 1/2 ((kap g)[p,q] - (g kap)[p,q]),  gt[p,q] = 2 (Ft[p,q] - Ft[q,p]) the gradient formula on the Fock matrix
// of the transformed table.  kap[a n + P] = kappa[a,P] (antisymmetric: the door has checked it), g[p + n q] the gradient at kappa = 0,
// Ft and sigma indexed as g.  One thread per entry of the square; the thread of p < q owns sigma[p,q] and sigma[q,p] = its exact
// negative, the thread of p == q the diagonal 0.0; the two chains run over k ascending from 0.0.
__global__ void __launch_bounds__(ORB_T) k_orb_sigma(const double *__restrict__ Ft, const double *__restrict__ g, const double *__restrict__ kap, int n,
                                                      double *__restrict__ sigma) {
  const int nn = n * n, e = blockIdx.x * ORB_T + threadIdx.x;
  if (e >= nn) return;
  const int p = e % n, q = e / n;
  if (p == q) { sigma[e] = 0.0; return; }
  if (p > q) return;
  double kg = 0.0, gk = 0.0;
  for (int k = 0; k < n; k++) kg = fma(kap[p * n + k], g[k + n * q], kg);
  for (int k = 0; k < n; k++) gk = fma(g[p + n * k], kap[k * n + q], gk);
  const double v = 2.0 * (Ft[p + n * q] - Ft[q + n * p]) + 0.5 * (kg - gk);
  sigma[p + n * q] = v + 0.0;
  sigma[q + n * p] = -v + 0.0;
}
