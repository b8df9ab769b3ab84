// rotate_kernels.h -- the integrals of a chem context in a new orbital basis (the rotation of generate_natorb_integrals, hci.f90:3683-3791)
// Textually included by sqmc_gpu.hip (one translation unit: the kernels share ChemDev and the packed index of chem_device.h); not a
// standalone header.
//
//   (PQ|RS)' = sum_abcd U_aP U_bQ U_cR U_dS (ab|cd),   h'_PQ = sum_ab U_aP U_bQ h_ab,   U_kp = rot[k norb + p], orbitals 0-based here
//
// Two half transformations over orbital pairs instead of the reference's four passes over the full tensor: the packed layout holds one
// member of every 8-fold class, and that member is all that is computed.  pair(p, q) = p (p + 1) / 2 + q for p >= q is the kernels' own
// numbering of the npair = norb (norb + 1) / 2 pairs; combine_2 is used only to address the context's integrals and the output.
//   k_rot<ROT_HALF1>, block rs = pair(r, s):  M[p][q] = (pq|rs) gathered through combine_2;  C = U^T M U;
//                                             work[pair(P, Q) npair + rs] = C[P][Q] for P >= Q
//   k_rot<ROT_HALF2>, block PQ = pair(P, Q):  M[r][s] = work[PQ npair + pair(max, min)];     C = U^T M U;
//                                             out[integral_index(P, Q, R, S)] = C[R][S] for R >= S, pair(R, S) <= PQ
//   k_rot<ROT_ONE>,   one block:              M[p][q] = h_pq = (p q | norb+1 norb+1);        C = U^T M U;
//                                             out[integral_index(P, Q, norb+1, norb+1)] = C[P][Q] for P >= Q; the nuclear energy is copied
// The work buffer is npair x npair doubles, a row per NEW pair PQ: half 2 reads its row contiguously, half 1 writes with stride npair.
//
// One body for all three.  LDS holds U, M and the intermediate T = M U, 3 norb^2 doubles sized by the context's norb (96 KB at 64 orbitals,
// which needs hipFuncAttributeMaxDynamicSharedMemorySize; 16 KB at 26).  M is symmetric, so both products have the form
// Z[i][j] = sum_k X[k][i] Y[k][j] with X and Y read along their rows: T = M^T U, C = U^T T.  A thread owns TM x TM tiles of Z in registers
// and adds the norb terms of an entry with fma in ascending k: every entry is written by one thread and has the same bits call to call
// (no atomics).  The explicit fma is the only contraction in the library (it is compiled with -ffp-contract=off): a product with an entry
// 0 or +-1 of U is exact, so the identity returns the input's bits and a signed permutation relabels them.

#define ROT_T 256                // threads of a block
enum { ROT_HALF1 = 0, ROT_HALF2 = 1, ROT_ONE = 2 };

// acc[i][j] = sum_k X[k n + i0 + i] Y[k n + j0 + j], k ascending; rows and columns beyond n read the last one (their sums are not stored)
template <int TM>
__device__ __forceinline__ void rot_xty(const double *__restrict__ X, const double *__restrict__ Y, int n, int i0, int j0, double (&acc)[TM][TM]) {
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

// grid: npair blocks (ROT_HALF1, ROT_HALF2) or one (ROT_ONE); dynamic LDS 3 norb^2 doubles.  src: the context's integrals (HALF1, ONE) or the
// work buffer (HALF2); dst: the work buffer (HALF1) or the output in the packed layout (HALF2, ONE)
template <int MODE, int TM>
__global__ void __launch_bounds__(ROT_T) k_rot(ChemDev dev, const double *__restrict__ rot, const double *__restrict__ src, double *__restrict__ dst, int norb) {
  extern __shared__ double rot_lds[];
  const int n = norb, nn = n * n, n1 = n + 1;
  const size_t npair = (size_t)n * (n + 1) / 2;
  double *U = rot_lds, *M = rot_lds + nn, *T = rot_lds + 2 * nn;
  const ChemTab &t = *dev.tab;          // combine_2 is read where it lies (L2): staging the table would cost the LDS of another block
  // the block's pair, hi >= lo
  const int blk = blockIdx.x;
  int hi = 0;
  while ((hi + 1) * (hi + 2) / 2 <= blk) hi++;
  const int lo = blk - hi * (hi + 1) / 2;
  for (int e = threadIdx.x; e < nn; e += ROT_T) {
    U[e] = rot[e];
    const int p = e / n, q = e - p * n;
    if (MODE == ROT_HALF1) M[e] = src[integral_index(t, p + 1, q + 1, hi + 1, lo + 1)];
    else if (MODE == ROT_ONE) M[e] = src[integral_index(t, p + 1, q + 1, n1, n1)];
    else { const int a = p > q ? p : q, b = p > q ? q : p; M[e] = src[(size_t)blk * npair + (size_t)(a * (a + 1) / 2 + b)]; }
  }
  __syncthreads();
  const int nt = (n + TM - 1) / TM;
  for (int tile = threadIdx.x; tile < nt * nt; tile += ROT_T) {      // T[a][Q] = sum_b M[b][a] U[b][Q]
    const int i0 = (tile / nt) * TM, j0 = (tile % nt) * TM;
    double acc[TM][TM];
    rot_xty<TM>(M, U, n, i0, j0, acc);
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TM; j++) if (i0 + i < n && j0 + j < n) T[(i0 + i) * n + j0 + j] = acc[i][j];
  }
  __syncthreads();
  for (int tile = threadIdx.x; tile < nt * nt; tile += ROT_T) {      // C[P][Q] = sum_a U[a][P] T[a][Q], the tiles that hold an entry to store
    const int i0 = (tile / nt) * TM, j0 = (tile % nt) * TM;
    if (j0 > i0 || (MODE == ROT_HALF2 && i0 > hi)) continue;
    double acc[TM][TM];
    rot_xty<TM>(U, T, n, i0, j0, acc);
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TM; j++) {
        const int P = i0 + i, Q = j0 + j;
        if (P >= n || Q > P) continue;
        const int pq = P * (P + 1) / 2 + Q;
        if (MODE == ROT_HALF1) dst[(size_t)pq * npair + blk] = acc[i][j];
        else if (MODE == ROT_ONE) dst[integral_index(t, P + 1, Q + 1, n1, n1)] = acc[i][j];
        else if (pq <= blk) dst[integral_index(t, hi + 1, lo + 1, P + 1, Q + 1)] = acc[i][j];
      }
  }
  if (MODE == ROT_ONE && threadIdx.x == 0) { const int ix = integral_index(t, n1, n1, n1, n1); dst[ix] = src[ix]; }
}
