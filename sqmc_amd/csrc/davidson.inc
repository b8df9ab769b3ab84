// davidson.inc -- the diagonally preconditioned Davidson of davidson_sparse (more_tools.f90:2018-2244; one-state twin
// davidson_sparse_single :3056-3230) with every vector resident in HBM: basis V, H V, the current best vectors W, H W and the
// correction vector never leave the device; the host sees only dot products (as per-block partial sums it adds up in block order)
// and diagonalises the small Krylov matrix.  Textually included by sqmc_gpu.hip behind abi_doors.inc (it launches k_spmv_wave on
// the plan's stream).
//
// The iteration is the reference's, so that the SAME state is tracked (a start in one symmetry sector stays there): start from
// v0 (Gram-Schmidt in order) or unit vectors on the first k rows; per sweep one correction vector per state,
// (H w - e w)/(e - H_ii) with -1 where the denominator vanishes (2131-2141), orthogonalised against the whole basis one vector after
// the other (modified Gram-Schmidt, 2146-2153); Krylov matrix diagonalised after every k additions (2170-2189); stop when the
// eigenvalues move by less than tol (epsilon = 1e-10, more_tools.f90:73) or the summed squared correction norms fall below 1e-12;
// the 50-vectors-per-state basis is recycled from the current best vectors (2107-2125).
//
// Where this leaves the reference.  The reference normalises every orthogonalised correction, also one that is zero or rounding
// noise (a start that already spans an invariant subspace: 1/sqrt(0), or a unit vector of noise that is not orthogonal to the basis),
// and it diagonalises only after every k additions, so with min(n, 50 k) not a multiple of k the last vectors are never used.  Here
//   - a correction that vanishes under the orthogonalisation (dv_breakdown) ends the iteration: the basis built so far is
//     diagonalised, and the result is returned only if its residuals say it is an eigen-solution, else SQMC_ERR_BREAKDOWN;
//   - a basis of n vectors spans everything: it is diagonalised whatever n mod k is, and that result is final;
//   - n_states == n is solved by the k x k matrix of the start vectors;
//   - a result reached through the reference's own criterion, summed |t|^2 < 1e-12, is returned only if its residuals bear that
//     criterion out, else SQMC_ERR_BREAKDOWN (the last correction was rounding noise above the level of dv_breakdown, and the last
//     diagonalisation left the state that had converged for a lower one).
// The iterates are the reference's, bit for bit what they were: the first three events end the iteration where the reference's next
// step is undefined, and the residual test changes no number, it only refuses a result.
//
// Sums: a dot product is a fixed tree -- lanes of a block by shuffles, blocks in index order --, the same on every run.

#define DV_TPB 256
#define DV_MAXB 1024
__device__ __forceinline__ double dv_block_sum(double v) {
  __shared__ double s_w[DV_TPB / 64];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                     // (a second call in one kernel reuses s_w)
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int q = 0; q < DV_TPB / 64; q++) t += s_w[q];
  return t;
}
__device__ __forceinline__ double dv_sum_partials(const double *__restrict__ part, int nb) {
  double c = 0.0;
  for (int q = threadIdx.x; q < nb; q += DV_TPB) c += part[q];
  return dv_block_sum(c);                              // every block adds the same numbers in the same tree: the same value in all of them
}
// part[j * nb + b] = this block's share of dot(A_j, x), j < m (A column-major, leading dimension n)
__global__ void __launch_bounds__(DV_TPB) dv_dots(const double *__restrict__ A, long long n, int m, const double *__restrict__ x, double *__restrict__ part) {
  const int nb = gridDim.x;
  for (int j = 0; j < m; j++) {
    const double *a = A + (long long)j * n;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)nb * DV_TPB) s += a[i] * x[i];
    s = dv_block_sum(s);
    if (threadIdx.x == 0) part[(long long)j * nb + blockIdx.x] = s;
  }
}
// t = (Hw - low w) / (low - diag), -1 where |low - diag| < 1e-8; part_res: dot(t, t); part_next: dot(t, v0) (the first Gram-Schmidt coefficient)
__global__ void __launch_bounds__(DV_TPB) dv_correction(const double *__restrict__ Hw, const double *__restrict__ w, double low, const double *__restrict__ diag,
                                                        double *__restrict__ t, long long n, const double *__restrict__ v0, double *__restrict__ part_res, double *__restrict__ part_next) {
  const int nb = gridDim.x;
  double r = 0.0, d = 0.0;
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)nb * DV_TPB) {
    const double den = low - diag[i];
    const double x = (fabs(den) < 1e-8) ? -1.0 : (Hw[i] - low * w[i]) / den;
    t[i] = x; r += x * x; if (v0) d += x * v0[i];
  }
  r = dv_block_sum(r); d = dv_block_sum(d);
  if (threadIdx.x == 0) { part_res[blockIdx.x] = r; if (part_next) part_next[blockIdx.x] = d; }
}
// one step of modified Gram-Schmidt: t -= c v_j with c = sum(part_in); part_out = dot(t, v_next) of the updated t (v_next = null: dot(t, t))
__global__ void __launch_bounds__(DV_TPB) dv_mgs_step(double *__restrict__ t, const double *__restrict__ vj, const double *__restrict__ part_in, long long n,
                                                      const double *__restrict__ v_next, double *__restrict__ part_out) {
  const int nb = gridDim.x;
  const double c = dv_sum_partials(part_in, nb);
  double d = 0.0;
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)nb * DV_TPB) {
    const double x = t[i] - c * vj[i];
    t[i] = x; d += x * (v_next ? v_next[i] : x);
  }
  d = dv_block_sum(d);
  if (threadIdx.x == 0) part_out[blockIdx.x] = d;
}
// out = t / sqrt(sum(part))
__global__ void __launch_bounds__(DV_TPB) dv_normalize(const double *__restrict__ t, const double *__restrict__ part, double *__restrict__ out, long long n) {
  const int nb = gridDim.x;
  const double s = 1.0 / sqrt(dv_sum_partials(part, nb));
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)nb * DV_TPB) out[i] = t[i] * s;
}
// t = v / |v| without a projection in front (the first start vector)
__global__ void __launch_bounds__(DV_TPB) dv_self_dot(const double *__restrict__ t, long long n, double *__restrict__ part) {
  double d = 0.0;
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * DV_TPB) d += t[i] * t[i];
  d = dv_block_sum(d);
  if (threadIdx.x == 0) part[blockIdx.x] = d;
}
// W[:, s] = sum_j A[:, j] y[j + m s], s < k (y on the device, column-major m x k)
__global__ void __launch_bounds__(DV_TPB) dv_combine(const double *__restrict__ A, long long n, int m, const double *__restrict__ y, int k, double *__restrict__ W) {
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * DV_TPB)
    for (int s = 0; s < k; s++) {
      double acc = 0.0;
      for (int j = 0; j < m; j++) acc += A[(long long)j * n + i] * y[j + m * s];
      W[(long long)s * n + i] = acc;
    }
}

// part_r[b], part_h[b]: this block's share of |Hw - e w|^2 and of |Hw|^2
__global__ void __launch_bounds__(DV_TPB) dv_residual(const double *__restrict__ Hw, const double *__restrict__ w, double e, long long n,
                                                      double *__restrict__ part_r, double *__restrict__ part_h) {
  double r = 0.0, h = 0.0;
  for (long long i = (long long)blockIdx.x * DV_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * DV_TPB) {
    const double x = Hw[i] - e * w[i];
    r += x * x; h += Hw[i] * Hw[i];
  }
  r = dv_block_sum(r); h = dv_block_sum(h);
  if (threadIdx.x == 0) { part_r[blockIdx.x] = r; part_h[blockIdx.x] = h; }
}

// Has the correction vanished under the orthogonalisation against m basis vectors?  before2, after2: its squared norm in front of and
// behind the m projections.  Each projection t -= (t.v_j) v_j rounds every element once in the product and once in the difference, and
// its coefficient comes from a dot product whose fixed tree (a strided serial part of at most a few terms, 6 shuffles, 4 waves, up to
// 1024 partials in 4 + 8 steps) commits fewer than 30 roundings on the way of a term: fewer than 32 units of u = 2^-53 per projection,
// relative to |t|.  Doubled for the two norms compared: 64 m u |t|.  What is left below that is what the projections themselves made,
// not a direction; zero and non-finite norms are below it by definition.
// An assumption, not a derivation, is the floor of 1 under |t|: t = (H w - e w)/(e - H_ii) is itself computed from the unit vector w,
// and the rounding it inherits is u |e| / |e - H_ii| per element, which is of the size of u only where the preconditioner's denominators
// are not small against |e| (below 1e-8 they are replaced by -1, which makes |t| >= 1).  With the floor the level is absolute, 64 m u,
// for |t| < 1: at most 1e-12 at m = 150, six orders under the |t| = 1e-6 at which the iteration stops anyway.
static bool dv_breakdown(double before2, double after2, int m) {
  const double level = 64.0 * (double)std::max(m, 1) * 1.1102230246251565e-16;
  return !(after2 > level * level * std::max(before2, 1.0));
}

// cyclic Jacobi on a symmetric m x m matrix (row-major a, destroyed); eigenvalues ascending in ev, eigenvectors in the columns of y (y[j + m s])
static void dv_small_eigh(int m, std::vector<double> &a, std::vector<double> &ev, std::vector<double> &y) {
  std::vector<double> V((size_t)m * m, 0.0);
  for (int i = 0; i < m; i++) V[(size_t)i * m + i] = 1.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < m; p++) { dia += a[(size_t)p * m + p] * a[(size_t)p * m + p]; for (int q = p + 1; q < m; q++) off += a[(size_t)p * m + q] * a[(size_t)p * m + q]; }
    if (off <= 1e-32 * (dia + off) || off == 0.0) break;
    for (int p = 0; p < m - 1; p++) for (int q = p + 1; q < m; q++) {
      const double apq = a[(size_t)p * m + q];
      if (apq == 0.0) continue;
      const double theta = (a[(size_t)q * m + q] - a[(size_t)p * m + p]) / (2.0 * apq);
      const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
      for (int r = 0; r < m; r++) {            // columns p, q
        const double arp = a[(size_t)r * m + p], arq = a[(size_t)r * m + q];
        a[(size_t)r * m + p] = cs * arp - sn * arq; a[(size_t)r * m + q] = sn * arp + cs * arq;
      }
      for (int r = 0; r < m; r++) {            // rows p, q
        const double apr = a[(size_t)p * m + r], aqr = a[(size_t)q * m + r];
        a[(size_t)p * m + r] = cs * apr - sn * aqr; a[(size_t)q * m + r] = sn * apr + cs * aqr;
      }
      for (int r = 0; r < m; r++) {
        const double vrp = V[(size_t)r * m + p], vrq = V[(size_t)r * m + q];
        V[(size_t)r * m + p] = cs * vrp - sn * vrq; V[(size_t)r * m + q] = sn * vrp + cs * vrq;
      }
    }
  }
  std::vector<int> ord(m);
  for (int i = 0; i < m; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int z) { return a[(size_t)x * m + x] < a[(size_t)z * m + z]; });
  ev.resize(m); y.assign((size_t)m * m, 0.0);
  for (int s = 0; s < m; s++) {
    ev[s] = a[(size_t)ord[s] * m + ord[s]];
    int big = 0;
    for (int j = 0; j < m; j++) { y[j + (size_t)m * s] = V[(size_t)j * m + ord[s]]; if (fabs(y[j + (size_t)m * s]) > fabs(y[big + (size_t)m * s])) big = j; }
    if (y[big + (size_t)m * s] < 0.0) for (int j = 0; j < m; j++) y[j + (size_t)m * s] = -y[j + (size_t)m * s];      // a fixed sign: largest component positive
  }
}

int sqmc_gpu_davidson(sqmc_spmv_plan *p, const double *diag, int32_t n_states, const double *v0, double tol, double *evals, double *evecs, int32_t *n_matvec) {
  if (!p || !diag || !evals || !evecs || n_states < 1) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  const long long n = p->n; const int k = n_states;
  if (k > n) return fail(SQMC_ERR_BAD_ARG, "more states than rows");
  if (n_matvec) *n_matvec = 0;
  if (n == 1) { evals[0] = diag[0]; evecs[0] = 1.0; return SQMC_OK; }
  const int iterations = (int)std::min<long long>(n, 50), m_max = k * iterations;
  const int niter = (int)std::min<long long>(n, (long long)m_max);
  hipStream_t st = p->st;
  const int nb = (int)std::min<long long>((n + DV_TPB - 1) / DV_TPB, DV_MAXB);
  DevScratch s(st);
  double *V = s.take<double>((size_t)n * m_max), *HV = s.take<double>((size_t)n * m_max), *W = s.take<double>((size_t)n * k), *HW = s.take<double>((size_t)n * k);
  double *t = s.take<double>(n), *dd = s.take<double>(n), *part = s.take<double>((size_t)(m_max + 2) * nb), *dy = s.take<double>((size_t)m_max * k);
  if (!s.ok()) return hip_fail("sqmc_gpu_davidson", s.err());
  HIPCHK(hipMemcpyAsync(dd, diag, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(V, 0, (size_t)n * m_max * 8, st));
  std::vector<double> hpart((size_t)(m_max + 2) * nb);
  double *part_a = part, *part_b = part + nb, *part_cols = part + 2 * nb;       // two alternating rows for the Gram-Schmidt chain, then one row per basis vector
  auto matvec = [&](const double *x, double *y) {
    hipLaunchKernelGGL(k_spmv_wave<0>, dim3((unsigned)((n + SPMV_ROWS_PER_BLOCK - 1) / SPMV_ROWS_PER_BLOCK)), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, st, p->d_ptr, p->d_col, p->d_val, x, y, n);
    if (n_matvec) (*n_matvec)++;
  };
  // orthogonalise t against V[:, 0..j_end) one after the other (part_a holds dot(t, V_0) on entry when j_end > 0), normalise into `out`
  auto mgs_into = [&](int j_end, double *out) -> const double * {
    double *pin = part_a, *pout = part_b;
    for (int j = 0; j < j_end; j++) {
      hipLaunchKernelGGL(dv_mgs_step, dim3(nb), dim3(DV_TPB), 0, st, t, V + (size_t)j * n, pin, n, (j + 1 < j_end) ? V + (size_t)(j + 1) * n : (const double *)nullptr, pout);
      std::swap(pin, pout);
    }
    if (j_end == 0) hipLaunchKernelGGL(dv_self_dot, dim3(nb), dim3(DV_TPB), 0, st, t, n, pin);
    hipLaunchKernelGGL(dv_normalize, dim3(nb), dim3(DV_TPB), 0, st, t, pin, out, n);
    return (const double *)pin;                  // the partial sums of |t|^2 that were normalised by
  };
  // host value of m dot products: partial rows part_cols[j][0..nb) summed in block order
  auto read_dots = [&](int m, std::vector<double> &out) -> int {
    HIPCHK(hipMemcpyAsync(hpart.data(), part_cols, (size_t)m * nb * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
    out.resize(m);
    for (int j = 0; j < m; j++) { double s = 0.0; for (int q = 0; q < nb; q++) s += hpart[(size_t)j * nb + q]; out[j] = s; }
    return SQMC_OK;
  };
  std::vector<double> hk((size_t)m_max * m_max, 0.0), low(k, 0.0), low_prev(k, INFINITY), res(k, 1.0), col, hnorm((size_t)nb);
  // ---- start vectors
  if (v0) {
    for (int i = 0; i < k; i++) {
      HIPCHK(hipMemcpyAsync(t, v0 + (size_t)i * n, n * 8, hipMemcpyHostToDevice, st));
      if (i > 0) hipLaunchKernelGGL(dv_dots, dim3(nb), dim3(DV_TPB), 0, st, V, n, 1, t, part_a);
      mgs_into(i, V + (size_t)i * n);
    }
  } else {
    std::vector<double> one(1, 1.0);
    for (int i = 0; i < k; i++) HIPCHK(hipMemcpyAsync(V + (size_t)i * n + i, one.data(), 8, hipMemcpyHostToDevice, st));
  }
  auto seed_block = [&]() -> int {          // hk[0..k, 0..k) and low from the first k basis vectors
    for (int j = 0; j < k; j++) {
      hipLaunchKernelGGL(dv_dots, dim3(nb), dim3(DV_TPB), 0, st, V, n, j + 1, HV + (size_t)j * n, part_cols);
      int r = read_dots(j + 1, col); if (r) return r;
      for (int i = 0; i <= j; i++) hk[(size_t)i * m_max + j] = hk[(size_t)j * m_max + i] = col[i];
      low[j] = col[j];
    }
    return SQMC_OK;
  };
  for (int i = 0; i < k; i++) matvec(V + (size_t)i * n, HV + (size_t)i * n);
  { int r = seed_block(); if (r) return r; }
  HIPCHK(hipMemcpyAsync(W, V, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(HW, HV, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st));
  bool converged = false, check = false;
  std::vector<double> a, ev, y;
  int m_ritz = k;                                        // W, HW and low stand for this many basis vectors
  // Rayleigh-Ritz on the first m basis vectors: low, W, HW
  auto ritz = [&](int m) -> int {
    a.assign((size_t)m * m, 0.0);
    for (int r = 0; r < m; r++) for (int c2 = 0; c2 < m; c2++) a[(size_t)r * m + c2] = hk[(size_t)r * m_max + c2];
    dv_small_eigh(m, a, ev, y);
    for (int s = 0; s < k; s++) low[s] = ev[s];
    HIPCHK(hipMemcpyAsync(dy, y.data(), (size_t)m * k * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dv_combine, dim3(nb), dim3(DV_TPB), 0, st, V, n, m, dy, k, W);
    hipLaunchKernelGGL(dv_combine, dim3(nb), dim3(DV_TPB), 0, st, HV, n, m, dy, k, HW);
    HIPCHK(hipStreamSynchronize(st));            // y is reused by the next diagonalisation
    m_ritz = m;
    return SQMC_OK;
  };
  if (k == n) { int r = ritz(k); if (r) return r; check = true; }      // the start vectors span everything
  for (long long it = k + 1; !check && it <= (long long)niter * 10; it++) {
    const int itc = (int)((it - 1) % niter) + 1;
    if (it > niter && itc == 1) {            // recycle the basis from the current best vectors
      HIPCHK(hipMemcpyAsync(V, W, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st)); HIPCHK(hipMemcpyAsync(HV, HW, (size_t)n * k * 8, hipMemcpyDeviceToDevice, st));
      int r = seed_block(); if (r) return r;
      m_ritz = k;
      continue;
    }
    const int i = (itc - 1) % k;
    hipLaunchKernelGGL(dv_correction, dim3(nb), dim3(DV_TPB), 0, st, HW + (size_t)i * n, W + (size_t)i * n, low[i], dd, t, n,
                       (itc - 1 > 0) ? V : (const double *)nullptr, part_cols, (itc - 1 > 0) ? part_a : (double *)nullptr);
    HIPCHK(hipMemcpyAsync(hpart.data(), part_cols, (size_t)nb * 8, hipMemcpyDeviceToHost, st));      // read below, behind the kernels that follow
    const double *pnorm = mgs_into(itc - 1, V + (size_t)(itc - 1) * n);
    HIPCHK(hipMemcpyAsync(hnorm.data(), pnorm, (size_t)nb * 8, hipMemcpyDeviceToHost, st));          // |t|^2 behind the projections
    matvec(V + (size_t)(itc - 1) * n, HV + (size_t)(itc - 1) * n);
    HIPCHK(hipStreamSynchronize(st));
    { double s = 0.0; for (int q = 0; q < nb; q++) s += hpart[q]; res[i] = s; }
    { double s = 0.0; for (int q = 0; q < k; q++) s += res[q]; if (s < 1.0e-12) converged = true; }
    { double s = 0.0; for (int q = 0; q < nb; q++) s += hnorm[q];
      if (dv_breakdown(res[i], s, itc - 1)) {          // nothing to add: what the basis in front of this vector gives is all there is
        if (itc - 1 > m_ritz) { int r = ritz(itc - 1); if (r) return r; }
        check = true; break;
      } }
    hipLaunchKernelGGL(dv_dots, dim3(nb), dim3(DV_TPB), 0, st, V, n, itc, HV + (size_t)(itc - 1) * n, part_cols);
    { int r = read_dots(itc, col); if (r) return r; }
    for (int j = 0; j < itc; j++) hk[(size_t)j * m_max + (itc - 1)] = hk[(size_t)(itc - 1) * m_max + j] = col[j];
    if (itc % k == 0 || itc == n) {
      { int r = ritz(itc); if (r) return r; }
      if (itc == n) { check = true; break; }       // n orthonormal vectors: the Krylov matrix is the matrix, nothing is left to add
      double move = 0.0;
      for (int s = 0; s < k; s++) move = std::max(move, fabs(low[s] - low_prev[s]));
      if (move < tol || converged) break;
      low_prev = low;
    }
  }
  if (check || converged) {
    // Return what the iteration ended on only if it is an eigen-solution by the reference's own criterion, summed |t|^2 < 1e-12.  With
    // t_i = r_i / (e - H_ii) that criterion says |r|^2 <= max_i (e - H_ii)^2 1e-12 <= 2 (e^2 + max H_ii^2) 1e-12, and e^2 <= |H w|^2 for
    // a unit w: |r|^2 <= 2e-12 (|H w|^2 + max H_ii^2).  A run that converged had this in front of its last diagonalisation, which
    // refines the state and does not enlarge its residual; a run that ended on an event above never got to ask.
    double dmax = 0.0; for (long long i = 0; i < n; i++) dmax = std::max(dmax, fabs(diag[i]));
    for (int s = 0; s < k; s++) {
      hipLaunchKernelGGL(dv_residual, dim3(nb), dim3(DV_TPB), 0, st, HW + (size_t)s * n, W + (size_t)s * n, low[s], n, part_a, part_b);
      HIPCHK(hipMemcpyAsync(hpart.data(), part_a, (size_t)2 * nb * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
      double r2 = 0.0, h2 = 0.0;
      for (int q = 0; q < nb; q++) { r2 += hpart[q]; h2 += hpart[(size_t)nb + q]; }
      const double allowed = 2.0e-12 * (h2 + dmax * dmax);
      if (!(r2 <= allowed) || !std::isfinite(low[s])) {
        char msg[200];
        snprintf(msg, sizeof msg, "Davidson: the iteration ended with state %d of %d not an eigen-solution (|Hx - ex|^2 = %.3g, allowed %.3g)", s + 1, k, r2, allowed);
        return fail(SQMC_ERR_BREAKDOWN, msg);
      }
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(evecs, W, (size_t)n * k * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  for (int s = 0; s < k; s++) evals[s] = low[s];
  return SQMC_OK;
}
