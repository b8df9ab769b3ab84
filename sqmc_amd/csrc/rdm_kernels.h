// rdm_kernels.h -- one-body reduced density matrix of an HCI wavefunction (get_1rdm, hci.f90:3198-3398; get_1rdm_with_pt, :3400-3551)
// Textually included by sqmc_gpu.hip (one translation unit: the kernels share ChemDev, det_key and h_any defined there); not a
// standalone header.
//
// rdm[p + norb r] = sum_sigma sum_i c_i c_k sign, k = determinant i with the sigma electron moved p -> r (p occupied in i; r empty or
// r = p), sign = (-1)^(occupied sigma orbitals strictly between p and r) = permutation_factor of the two sigma strings; 0-based.
//
// Owner computes, no atomics: a block owns one (p, r, sigma) and one chunk of RDM_CHUNK consecutive determinants of the list in rank
// order.  Its threads stride over the chunk; a thread tests the two bits, forms k, looks its rank up in the sorted ranks by binary
// search and adds the term to a private sum; the block adds the private sums by the fixed shuffle / LDS tree of k_pt2_terms and
// writes partial[chunk][p][r][sigma].  k_rdm_sum then adds the chunks in chunk order, up before dn.  Which thread meets which
// determinant depends on the rank order alone, so an entry has the same bits run to run and for any order of the caller's list.
// The bit tests run over every determinant for every (p, r), about norb^2 / (n_occ n_virt) times more than the pairs that pass;
// the searches, which dominate, are not multiplied.
//
// The PT part (<0|rho|1> + <1|rho|0>): the reference searches the connected list first and the variational list second (:3488-3491).
// A variational determinant with c != 0 always occupies its own slot of the connected list and one with c = 0 contributes nothing,
// so the variational pass above (which searches the variational list alone) and a pass over the connected determinants OUTSIDE the
// variational space give the same matrix.  k_rdm_psi1 writes psi1_a = (sum_j H_aj c_j) / (E_var - H_aa) once per connected
// determinant of a slice, 0 for a inside the variational space, and its rank; k_rdm_pt is k_rdm_var with the search going to the
// slice's ranks and the term sign c_i psi1_a; k_rdm_pt_sum adds a slice's chunks to T[p][r]; k_rdm_pt_final writes
// rdm(p, r) = var(p, r) + (T(p, r) + T(r, p)).  No <1|rho|1> term and no renormalisation: the trace stays nelec sum c^2.
// Active-space masks (sqmc_gpu_hci_set_active_space) are generator state of the context and shape the connected space as they stand.

#define RDM_T 256                // threads of a block
#define RDM_CHUNK 1024           // determinants of a block's chunk (four per thread)

// sorted order: su/sd/sc[j] = the caller's determinant perm[j] and its coefficient
__global__ void __launch_bounds__(TPB) k_rdm_gather(const u32 *__restrict__ perm, const u64 *__restrict__ vu, const u64 *__restrict__ vd, const double *__restrict__ vc,
                                                    u64 *__restrict__ su, u64 *__restrict__ sd, double *__restrict__ sc, long long n) {
  const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
  if (j >= n) return;
  const u32 i = perm[j];
  su[j] = vu[i]; sd[j] = vd[i]; sc[j] = vc[i];
}
// two equal ranks side by side in the sorted list: a repeated determinant
__global__ void __launch_bounds__(TPB) k_rdm_repeats(const u64 *__restrict__ skey, long long n, int *__restrict__ flag) {
  const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
  if (j + 1 < n && skey[j] == skey[j + 1]) atomicOr(flag, 1);
}
// the block's sum by the tree of k_pt2_terms: 64-lane shuffles, then the wavefronts' sums left to right
__device__ __forceinline__ void rdm_block_store(double acc, double *__restrict__ out) {
  __shared__ double red[RDM_T / 64];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { double v = 0.0; for (int q = 0; q < RDM_T / 64; q++) v += red[q]; *out = v; }
}
// (-1)^(bits of s strictly between positions p and r)
__device__ __forceinline__ double rdm_sign(u64 s, int p, int r) {
  const int lo = p < r ? p : r, hi = p < r ? r : p;
  const u64 between = maskr64(hi) & ~maskr64(lo + 1);
  return (popc64(s & between) & 1) ? -1.0 : 1.0;
}
// PT = false: tkey / tval = the list's own sorted ranks and coefficients (nt = n).  PT = true: the ranks and psi1 of a slice of the
// connected space.  grid (chunks, norb * norb * 2); sym: norb labels or null
template <bool PT>
__global__ void __launch_bounds__(RDM_T) k_rdm_terms(ChemDev dev, const u64 *__restrict__ su, const u64 *__restrict__ sd, const double *__restrict__ sc, long long n,
                                                     const u64 *__restrict__ tkey, const double *__restrict__ tval, long long nt, int norb,
                                                     const unsigned char *__restrict__ sym, double *__restrict__ partial) {
  const int pair = blockIdx.y, sigma = pair & 1, r = (pair >> 1) % norb, p = (pair >> 1) / norb;
  double *out = partial + (size_t)blockIdx.x * gridDim.y + pair;
  if ((PT && p == r) || (sym && sym[p] != sym[r])) { if (threadIdx.x == 0) *out = 0.0; return; }      // the same for every thread of the block
  const long long j0 = (long long)blockIdx.x * RDM_CHUNK, j1 = (j0 + RDM_CHUNK < n) ? j0 + RDM_CHUNK : n;
  const u64 bp = bit64(p), br = bit64(r);
  double acc = 0.0;
  for (long long j = j0 + threadIdx.x; j < j1; j += RDM_T) {
    const u64 u = su[j], d = sd[j], s = sigma ? d : u;
    if (!(s & bp)) continue;
    if (p == r) { const double ci = sc[j]; acc += ci * ci; continue; }
    if (s & br) continue;
    const u64 s2 = (s ^ bp) | br;
    const u64 key = sigma ? det_key(dev, u, s2) : det_key(dev, s2, d);
    long long lo = 0, hi = nt;                         // first rank >= key
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (tkey[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo >= nt || tkey[lo] != key) continue;
    acc += rdm_sign(s, p, r) * sc[j] * tval[lo];
  }
  rdm_block_store(acc, out);
}
// one thread per (p, r): chunks in chunk order, up then dn.  flat index of the output: p + norb r
__global__ void __launch_bounds__(TPB) k_rdm_sum(const double *__restrict__ partial, int nchunks, int norb, double *__restrict__ rdm) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= norb * norb) return;
  const size_t stride = (size_t)norb * norb * 2;
  double a = 0.0, b = 0.0;
  for (int q = 0; q < nchunks; q++) a += partial[q * stride + 2 * e];
  for (int q = 0; q < nchunks; q++) b += partial[q * stride + 2 * e + 1];
  rdm[(e / norb) + norb * (e % norb)] = a + b;
}
// psi1 and rank of every connected determinant of a slice; vkeys: the sorted ranks of the variational determinants
__global__ void __launch_bounds__(TPB) k_rdm_psi1(ChemDev dev, const u64 *__restrict__ cu, const u64 *__restrict__ cd, const double *__restrict__ num, long long n,
                                                  const u64 *__restrict__ vkeys, long long nv, double e_var, u64 *__restrict__ ckey, double *__restrict__ psi1) {
  __shared__ ChemTab t;
  stage_tab(&t, dev.tab, dev.tab_words);
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const u64 u = cu[i], d = cd[i];
  const u64 key = det_key(dev, u, d);
  long long lo = 0, hi = nv;
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (vkeys[mid] < key) lo = mid + 1; else hi = mid; }
  double v = 0.0;
  if (!(lo < nv && vkeys[lo] == key)) v = num[i] / (e_var - h_any(t, dev.integrals, u, d, u, d));
  ckey[i] = key; psi1[i] = v;
}
// T[p][r] += the slice's chunks in chunk order, up then dn (T in the layout of partial's pairs: (p norb + r))
__global__ void __launch_bounds__(TPB) k_rdm_pt_sum(const double *__restrict__ partial, int nchunks, int norb, double *__restrict__ T) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= norb * norb) return;
  const size_t stride = (size_t)norb * norb * 2;
  double a = 0.0, b = 0.0;
  for (int q = 0; q < nchunks; q++) a += partial[q * stride + 2 * e];
  for (int q = 0; q < nchunks; q++) b += partial[q * stride + 2 * e + 1];
  T[e] = T[e] + (a + b);
}
__global__ void __launch_bounds__(TPB) k_rdm_pt_final(const double *__restrict__ var, const double *__restrict__ T, int norb, double *__restrict__ rdm) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= norb * norb) return;
  const int p = e / norb, r = e % norb;
  rdm[p + norb * r] = var[p + norb * r] + (T[p * norb + r] + T[r * norb + p]);
}
