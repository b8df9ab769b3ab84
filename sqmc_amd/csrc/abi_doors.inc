// abi_doors.inc -- C-ABI batch doors, HCI, Hamiltonian build and SpMV entry points (inside extern "C")
// Textually included by sqmc_gpu.hip (one translation unit: the kernels share the ChemTab LDS
// image, the walker SoA types and the launch helpers defined there); not a standalone header.

// ---------------------------------------------------------------- batch doors
extern "C++" {
template <class K>
static int ham_batch(K kern, const char *who, sqmc_gpu_ctx *c, int64_t n, const uint64_t *iu, const uint64_t *id, const uint64_t *ju, const uint64_t *jd, double *h) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (n <= 0) return SQMC_OK;
  DevScratch s(c->st);
  u64 *d[4]; const uint64_t *src[4] = {iu, id, ju, jd};
  for (int k = 0; k < 4; k++) d[k] = s.take<u64>(n);
  double *dh = s.take<double>(n);
  if (!s.ok()) return hip_fail(who, s.err());
  for (int k = 0; k < 4; k++) HIPCHK(hipMemcpy(d[k], src[k], n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kern, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, d[0], d[1], d[2], d[3], dh, (long long)n);
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipMemcpy(h, dh, n * 8, hipMemcpyDeviceToHost));
  return SQMC_OK;
}
}
int sqmc_gpu_hamiltonian_batch(sqmc_gpu_ctx *c, int64_t n, const uint64_t *iu, const uint64_t *id, const uint64_t *ju, const uint64_t *jd, double *h) {
  return ham_batch(k_ham_batch, "sqmc_gpu_hamiltonian_batch", c, n, iu, id, ju, jd, h);
}
int sqmc_gpu_hamiltonian_chem_batch(sqmc_gpu_ctx *c, int64_t n, const uint64_t *iu, const uint64_t *id, const uint64_t *ju, const uint64_t *jd, double *h) {
  return ham_batch(k_ham_chem_batch, "sqmc_gpu_hamiltonian_chem_batch", c, n, iu, id, ju, jd, h);
}

// Rows of the sparse Hamiltonian of a sorted determinant list on the device, as generate_sparse_ham_chem_upper_triangular stores
// them (diagonal first, then the columns j < i ascending; 1-based indices): counts, offsets, indices, values and the total.
// Default: candidates from string groups (hbuild_kernels.h), cost ~ sum of group sizes; SQMC_HAM_ALLPAIRS=1: every pair tested
// (k_build_ham), the cross-check of the tests.  du, dd: the list on the device; up, dn: the same on the host.
// The rows go to `out` (didx, dval); every other buffer allocated here is released before returning.
static ScanWork scan_work(u64 *state, long long tiles) { ScanWork sw; sw.state = state; sw.ticket = (u32 *)(state + tiles); sw.cap_tiles = tiles; sw.self_clear = true; return sw; }
static int ham_rows_dev(sqmc_gpu_ctx *c, int64_t n, const uint64_t *up, const uint64_t *dn, const u64 *du, const u64 *dd, u64 *dcnt, u64 *doff, u64 *dtot,
                        ScanWork &sw, DevScratch &out, u64 *total_out, long long **didx_out, double **dval_out) {
  const char *who = "sparse Hamiltonian rows";
  hipStream_t st = c->st;
  static const bool allpairs = getenv("SQMC_HAM_ALLPAIRS") != nullptr;
  if (allpairs || c->htab.sys_type != 0 || n < 64) {
    hipLaunchKernelGGL(k_build_ham, dim3(nblk(n)), dim3(TPB), 0, st, c->dev, du, dd, (long long)n, 0, dcnt, doff, (long long *)nullptr, (double *)nullptr);
    device_excl_scan_u64(dcnt, doff, n, dtot, sw, st);
    u64 total = 0;
    HIPCHK(hipMemcpyAsync(&total, dtot, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
    long long *didx = out.take<long long>(total + 1); double *dval = out.take<double>(total + 1);
    if (!out.ok()) return hip_fail(who, out.err());
    hipLaunchKernelGGL(k_build_ham, dim3(nblk(n)), dim3(TPB), 0, st, c->dev, du, dd, (long long)n, 1, dcnt, doff, didx, dval);
    HIPCHK(hipGetLastError());
    *total_out = total; *didx_out = didx; *dval_out = dval;
    return SQMC_OK;
  }
  // ---- host: distinct strings, string ids, the two groupings (O(n log n) on 2n words; everything that scales with the matrix is on the device)
  std::vector<u64> S(2 * (size_t)n);
  for (int64_t i = 0; i < n; i++) { S[2 * i] = up[i]; S[2 * i + 1] = dn[i]; }
  std::sort(S.begin(), S.end()); S.erase(std::unique(S.begin(), S.end()), S.end());
  const int NS = (int)S.size();
  std::vector<u32> sid_up(n), sid_dn(n), ulo(NS, 0), uhi(NS, 0), dlo(NS + 1, 0), dhi(NS, 0), perm_d(n);
  for (int64_t i = 0; i < n; i++) {
    sid_up[i] = (u32)(std::lower_bound(S.begin(), S.end(), (u64)up[i]) - S.begin());
    sid_dn[i] = (u32)(std::lower_bound(S.begin(), S.end(), (u64)dn[i]) - S.begin());
    const u32 a = sid_up[i];
    if (uhi[a] == 0) ulo[a] = (u32)i;                 // the list is sorted by up: one contiguous range per alpha string
    uhi[a] = (u32)i + 1;
    dhi[sid_dn[i]]++;
  }
  { u32 acc = 0; for (int s2 = 0; s2 < NS; s2++) { const u32 cn = dhi[s2]; dlo[s2] = acc; acc += cn; dhi[s2] = dlo[s2]; } }
  for (int64_t i = 0; i < n; i++) perm_d[dhi[sid_dn[i]]++] = (u32)i;      // ascending inside every beta group
  DevScratch s(st);
  u64 *dS = s.take<u64>(NS), *ncnt = s.take<u64>(NS + 1), *nptr = s.take<u64>(NS + 1);
  u32 *dsu = s.take<u32>(n), *dsd = s.take<u32>(n), *dulo = s.take<u32>(NS), *duhi = s.take<u32>(NS), *ddlo = s.take<u32>(NS), *ddhi = s.take<u32>(NS), *dperm = s.take<u32>(n);
  // ---- strings one excitation away
  const long long tiles_s = (NS + SCAN_TILE - 1) / SCAN_TILE + 1;
  u64 *dts_s = s.take<u64>(tiles_s + 1);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemcpy(dS, S.data(), NS * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dsu, sid_up.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dsd, sid_dn.data(), n * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dulo, ulo.data(), NS * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(duhi, uhi.data(), NS * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(ddlo, dlo.data(), NS * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ddhi, dhi.data(), NS * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dperm, perm_d.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(dts_s, 0, (tiles_s + 1) * 8, st));
  ScanWork sws = scan_work(dts_s, tiles_s);
  hipLaunchKernelGGL(k_str_nbr, dim3(nblk(NS)), dim3(TPB), 0, st, (const u64 *)dS, NS, 0, ncnt, (const u64 *)nptr, (u32 *)nullptr);
  device_excl_scan_u64(ncnt, nptr, NS, nptr + NS, sws, st);
  u64 nn = 0; HIPCHK(hipMemcpyAsync(&nn, nptr + NS, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  u32 *dnbr = s.take<u32>(nn + 1);
  // ---- candidates: count, offsets, words
  u64 *ccnt = s.take<u64>(n), *coff = s.take<u64>(n);
  if (!s.ok()) return hip_fail(who, s.err());
  hipLaunchKernelGGL(k_str_nbr, dim3(nblk(NS)), dim3(TPB), 0, st, (const u64 *)dS, NS, 1, ncnt, (const u64 *)nptr, dnbr);
  HamIdx x; x.S = dS; x.NS = NS; x.sid_up = dsu; x.sid_dn = dsd; x.ulo = dulo; x.uhi = duhi; x.dlo = ddlo; x.dhi = ddhi; x.perm_d = dperm; x.nptr = nptr; x.nbr = dnbr;
  hipLaunchKernelGGL(k_ham_candidates, dim3(nblk(n)), dim3(TPB), 0, st, x, du, dd, (long long)n, c->htab.time_sym, 0, ccnt, (const u64 *)coff, (u64 *)nullptr);
  device_excl_scan_u64(ccnt, coff, n, dtot, sw, st);
  u64 m = 0; HIPCHK(hipMemcpyAsync(&m, dtot, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  u64 *keep = nullptr, *P = nullptr; double *hv = nullptr;
  u64 ptotal = 0;
  u64 *sorted = nullptr;
  if (m > 0) {
    u64 *words = s.take<u64>(m), *walt = s.take<u64>(m); keep = s.take<u64>(m); P = s.take<u64>(m); hv = s.take<double>(m);
    const long long nt = (long long)((m + RS_TILE - 1) / RS_TILE);
    u32 *hist = s.take<u32>((size_t)RS_MAX_RADIX * (nt + 1)), *rowtot = s.take<u32>(RS_MAX_RADIX);
    const long long tiles_m = (long long)((m + SCAN_TILE - 1) / SCAN_TILE + 1);
    u64 *dts_m = s.take<u64>(tiles_m + 1);
    if (!s.ok()) return hip_fail(who, s.err());
    hipLaunchKernelGGL(k_ham_candidates, dim3(nblk(n)), dim3(TPB), 0, st, x, du, dd, (long long)n, c->htab.time_sym, 1, ccnt, (const u64 *)coff, words);
    int kb = 1; while ((1ll << kb) < n) kb++;                       // row and column: 32 + kb bits, rows are contiguous already but the digits of a column pass scramble them
    SortWork so; so.k_alt = walt; so.v_alt = nullptr; so.hist = hist; so.rowtot = rowtot; so.cap = (long long)m;
    sorted = words; u32 *nov = nullptr;
    // columns first (kb bits at bit 0), then rows (kb bits at bit 32): two LSD sorts = one sort on (row, column)
    device_radix_sort(sorted, nov, (long long)m, kb, so, st, 0);
    device_radix_sort(sorted, nov, (long long)m, kb, so, st, 32);
    hipLaunchKernelGGL(k_ham_eval, dim3(nblk((long long)m)), dim3(TPB), 0, st, c->dev, du, dd, (const u64 *)sorted, (long long)m, hv, keep);
    HIPCHK(hipMemsetAsync(dts_m, 0, (tiles_m + 1) * 8, st));
    ScanWork swm = scan_work(dts_m, tiles_m);
    device_excl_scan_u64(keep, P, (long long)m, dtot, swm, st);
    HIPCHK(hipMemcpyAsync(&ptotal, dtot, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  }
  const u64 total = (u64)n + ptotal;
  long long *didx = out.take<long long>(total + 1); double *dval = out.take<double>(total + 1);
  if (!out.ok()) return hip_fail(who, out.err());
  hipLaunchKernelGGL(k_ham_rows, dim3(nblk(n)), dim3(TPB), 0, st, c->dev, du, dd, (long long)n, (const u64 *)coff, (const u64 *)P, (long long)m, ptotal, dcnt, doff, didx, dval);
  if (m > 0) hipLaunchKernelGGL(k_ham_place, dim3(nblk((long long)m)), dim3(TPB), 0, st, (const u64 *)sorted, (const double *)hv, (const u64 *)keep, (const u64 *)P, (long long)m, didx, dval);
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
  *total_out = total; *didx_out = didx; *dval_out = dval;
  return SQMC_OK;
}

// the sorted determinant list, its row counts / offsets and the scan state that both sparse-Hamiltonian doors hand to ham_rows_dev
struct HamListDev { u64 *du, *dd, *dcnt, *doff, *dtot; ScanWork sw; };
static int ham_list_dev(sqmc_gpu_ctx *c, const char *who, int64_t n, const uint64_t *up, const uint64_t *dn, int n_tot, DevScratch &s, HamListDev &L) {
  for (long long i = 1; i < n; i++)
    if (!(up[i - 1] < up[i] || (up[i - 1] == up[i] && dn[i - 1] < dn[i]))) return fail(SQMC_ERR_BAD_ARG, "determinant list must be strictly sorted by (up,dn)");
  const long long tiles = (n + SCAN_TILE - 1) / SCAN_TILE + 1;
  L.du = s.take<u64>(n); L.dd = s.take<u64>(n); L.dcnt = s.take<u64>(n); L.doff = s.take<u64>(n); L.dtot = s.take<u64>(n_tot);
  u64 *dts = s.take<u64>(tiles + 1);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemcpy(L.du, up, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(L.dd, dn, n * 8, hipMemcpyHostToDevice));
  L.sw = scan_work(dts, tiles);
  return SQMC_OK;
}

int sqmc_gpu_build_sparse_ham(sqmc_gpu_ctx *c, int64_t n, const uint64_t *up, const uint64_t *dn, int64_t *out_nnz,
                              int64_t **out_row_counts, int64_t **out_indices, double **out_values) {
  if (!c || !out_nnz || !out_row_counts || !out_indices || !out_values || n <= 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (c->htab.sys_type == 3 && c->htab.hk_sym)
    return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_build_sparse_ham is not built for hubbardk with space_sym: the matrix among representatives is assembled from sqmc_gpu_hci_connections in raw mode");
  hipStream_t st = c->st;
  DevScratch s(st); HamListDev L;
  int rh = ham_list_dev(c, "sqmc_gpu_build_sparse_ham", n, up, dn, 1, s, L);
  if (rh) return rh;
  u64 total = 0; long long *didx; double *dval;
  if ((rh = ham_rows_dev(c, n, up, dn, L.du, L.dd, L.dcnt, L.doff, L.dtot, L.sw, s, &total, &didx, &dval))) return rh;
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
  HostOut h;
  int64_t *rc = h.take<int64_t>(n), *ix = h.take<int64_t>(total + 1); double *vl = h.take<double>(total + 1);
  HIPCHK(hipMemcpy(rc, L.dcnt, n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(ix, didx, total * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(vl, dval, total * 8, hipMemcpyDeviceToHost));
  *out_nnz = (int64_t)total; h.commit(rc, out_row_counts); h.commit(ix, out_indices); h.commit(vl, out_values);
  return SQMC_OK;
}

// the matvec plan with its device buffers: those live in `mem` until sqmc_gpu_spmv_free
struct SpmvPlanOwned : sqmc_spmv_plan { DevScratch mem; };
static int spmv_plan_new(int64_t n, long long nnz_full, SpmvPlanOwned **out) {
  SpmvPlanOwned *p = new SpmvPlanOwned(); p->n = n; p->nnz_full = nnz_full;
  if (hipError_t e = hipStreamCreate(&p->st)) { delete p; return hip_fail("spmv plan", e); }
  p->mem.stream = p->st;
  p->d_ptr = p->mem.take<int>(n + 1); p->d_col = p->mem.take<int>(nnz_full + 1); p->d_val = p->mem.take<double>(nnz_full + 1);
  p->d_x = p->mem.take<double>(n); p->d_y = p->mem.take<double>(n);
  if (!p->mem.ok()) { const hipError_t e = p->mem.err(); sqmc_gpu_spmv_free(p); return hip_fail("spmv plan", e); }
  *out = p;
  return SQMC_OK;
}

// The sparse Hamiltonian of a sorted determinant list built on the device AND left there as a
// matvec plan: what generate_sparse_ham_chem_upper_triangular + davidson_sparse's matvec need,
// without the matrix crossing PCIe twice or being expanded on the host.  diag[n] (the Davidson
// preconditioner) and the number of stored (upper-triangular) nonzeros come back to the host.
int sqmc_gpu_build_spmv_plan(sqmc_gpu_ctx *c, int64_t n, const uint64_t *up, const uint64_t *dn, sqmc_spmv_plan **plan, double *diag, int64_t *out_nnz) {
  if (!c || !plan || !diag || !out_nnz || n <= 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (c->htab.sys_type == 3 && c->htab.hk_sym) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_build_spmv_plan is not built for hubbardk with space_sym (see sqmc_gpu_build_sparse_ham)");
  const char *who = "sqmc_gpu_build_spmv_plan";
  hipStream_t st = c->st;
  std::unique_ptr<sqmc_spmv_plan, int (*)(sqmc_spmv_plan *)> guard(nullptr, sqmc_gpu_spmv_free);      // freed behind s, whose destructor waits for the kernels that write the plan
  DevScratch s(st); HamListDev L;
  int rh = ham_list_dev(c, who, n, up, dn, 2, s, L);
  if (rh) return rh;
  u64 *dcnt = L.dcnt, *doff = L.doff, *dtot = L.dtot;
  u64 total = 0; long long *didx; double *dval;
  if ((rh = ham_rows_dev(c, n, up, dn, L.du, L.dd, dcnt, doff, dtot, L.sw, s, &total, &didx, &dval))) return rh;
  const long long n_strict = (long long)total - n, nnz_full = (long long)total + n_strict;
  if (nnz_full >= (1ll << 31)) return fail(SQMC_ERR_UNSUPPORTED, "more than 2^31 expanded nonzeros");
  // transpose bookkeeping
  const long long ntile_sort = (long long)((total + RS_TILE - 1) / RS_TILE);
  u64 *dkeys = s.take<u64>(total), *dkeys_alt = s.take<u64>(total); u32 *dvals = s.take<u32>(total), *dvals_alt = s.take<u32>(total);
  u32 *drowof = s.take<u32>(total), *dcolcount = s.take<u32>(n + 1); u64 *drowlen = s.take<u64>(n), *dptr64 = s.take<u64>(n);
  u64 *dcolc = s.take<u64>(n), *dcolstart = s.take<u64>(n);
  u32 *dhist = s.take<u32>((size_t)RS_MAX_RADIX * (ntile_sort + 1)), *drowtot = s.take<u32>(RS_MAX_RADIX);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemsetAsync(dcolcount, 0, (n + 1) * 4, st));
  hipLaunchKernelGGL(k_csr_keys, dim3(nblk(n)), dim3(TPB), 0, st, dcnt, doff, didx, dkeys, dvals, drowof, dcolcount, (long long)n);
  hipLaunchKernelGGL(k_csr_rowlen, dim3(nblk(n)), dim3(TPB), 0, st, dcnt, dcolcount, drowlen, dcolc, (long long)n);
  device_excl_scan_u64(drowlen, dptr64, n, dtot, L.sw, st);
  device_excl_scan_u64(dcolc, dcolstart, n, dtot + 1, L.sw, st);
  int kb = 1; while ((1ll << kb) <= n) kb++;                      // keys are column indices 0..n (n = the diagonal marker)
  SortWork so; so.k_alt = dkeys_alt; so.v_alt = dvals_alt; so.hist = dhist; so.rowtot = drowtot; so.cap = (long long)total;
  u64 *sk = dkeys; u32 *sv = dvals;
  device_radix_sort(sk, sv, (long long)total, kb, so, st);
  SpmvPlanOwned *p = nullptr;
  if ((rh = spmv_plan_new(n, nnz_full, &p))) return rh;
  guard.reset(p);
  double *ddiag = s.take<double>(n);
  if (!s.ok()) return hip_fail(who, s.err());
  hipLaunchKernelGGL(k_csr_fill_stored, dim3(nblk(n + 1)), dim3(TPB), 0, st, dcnt, doff, didx, dval, dptr64, p->d_ptr, p->d_col, p->d_val, ddiag, (long long)n, nnz_full);
  if (n_strict > 0)
    hipLaunchKernelGGL(k_csr_fill_transposed, dim3(nblk(n_strict)), dim3(TPB), 0, st, sk, sv, drowof, dval, dcnt, dptr64, dcolstart, p->d_col, p->d_val, (long long)n, n_strict);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(diag, ddiag, n * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  *out_nnz = (int64_t)total; *plan = guard.release();
  return SQMC_OK;
}

// the three proposal doors: `width` children per walker (the heat-bath kernel proposes two)
extern "C++" {
template <class K>
static int propose_batch(K kern, const char *who, int width, sqmc_gpu_ctx *c, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                         uint64_t *ju, uint64_t *jd, double *wj, int32_t *seeds_after) {
  if (n <= 0) return SQMC_OK;
  std::vector<u64> s(n);
  for (long long i = 0; i < n; i++) s[i] = (((u64)seeds[4 * i] << 36) + ((u64)seeds[4 * i + 1] << 24) + ((u64)seeds[4 * i + 2] << 12) + (u64)seeds[4 * i + 3]) & SQ_MASK48;
  const long long nw = width * n;
  DevScratch m(c->st);
  u64 *du = m.take<u64>(n), *dd = m.take<u64>(n), *ds = m.take<u64>(n), *dju = m.take<u64>(nw), *djd = m.take<u64>(nw), *dso = m.take<u64>(n); double *dw = m.take<double>(nw);
  if (!m.ok()) return hip_fail(who, m.err());
  HIPCHK(hipMemcpy(du, up, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dd, dn, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ds, s.data(), n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kern, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, du, dd, ds, dju, djd, dw, dso, (long long)n, tau);
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipMemcpy(ju, dju, nw * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(jd, djd, nw * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(wj, dw, nw * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(s.data(), dso, n * 8, hipMemcpyDeviceToHost));
  for (long long i = 0; i < n; i++) { u64 x = s[i]; seeds_after[4 * i] = (int)((x >> 36) & 4095); seeds_after[4 * i + 1] = (int)((x >> 24) & 4095);
    seeds_after[4 * i + 2] = (int)((x >> 12) & 4095); seeds_after[4 * i + 3] = (int)(x & 4095); }
  return SQMC_OK;
}
}
int sqmc_gpu_propose_batch(sqmc_gpu_ctx *c, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                           uint64_t *ju, uint64_t *jd, double *wj, int32_t *seeds_after) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  return propose_batch(k_propose_batch, "sqmc_gpu_propose_batch", 1, c, n, tau, up, dn, seeds, ju, jd, wj, seeds_after);
}

int sqmc_gpu_set_heatbath_tables(sqmc_gpu_ctx *c, const sqmc_heatbath_tables *t) {
  abandon_head(c);          // a head enqueued with one walker slot per child must not meet a tail that counts two (a sharded run's pipelined head too)
  if (!c || !t) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (c->dev.cs.on) return fail(SQMC_ERR_BAD_ARG, "the context already proposes by Cauchy-Schwarz (sqmc_gpu_setup_cauchy_schwarz)");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "the efficient heat-bath proposal is a 'chem' proposal");
  if (c->psit_shard) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit with proposal_method fast_heatbath is not built");      // as sqmc_gpu_set_hf_to_psit_shard refuses the other order
  if (t->norb != c->htab.norb) return fail(SQMC_ERR_BAD_ARG, "norb of the tables differs from the context's");
  const int n = t->norb; const long long npairs = ((long long)n * (n - 1)) / 2 + n;
  if (t->size_same != (npairs - 1) * n * n + (long long)(n - 1) * n + n || t->size_opposite != (long long)n * n * n * n)
    return fail(SQMC_ERR_BAD_ARG, "size_same / size_opposite are not same_index(norb,...) / opposite_index(norb,...)");
  HbDev hb; memset(&hb, 0, sizeof(hb));
  hb.norb = n; hb.npairs = (int)npairs;
  int r;
  if ((r = hb_upload(c, 0, t->one_orbital_probabilities, (size_t)n, &hb.one))) return r;
  { std::vector<double> two((size_t)4 * n * n);        // (i,j) column-major -> [i][j]
    for (int i = 0; i < 2 * n; i++) for (int j = 0; j < 2 * n; j++) two[(size_t)i * 2 * n + j] = t->two_orbital_probabilities[(size_t)i + (size_t)2 * n * j];
    if ((r = hb_upload(c, 1, two.data(), two.size(), &hb.two))) return r; }
  { auto a = hb_transpose3(t->three_orbital_probabilities_same_spin, n); if ((r = hb_upload(c, 2, a.data(), a.size(), &hb.three_same))) return r; }
  { auto a = hb_transpose3(t->three_orbital_probabilities_opposite_spin, n); if ((r = hb_upload(c, 3, a.data(), a.size(), &hb.three_opp))) return r; }
  { auto a = hb_transpose3(t->J_three_orbital_probabilities_same_spin, n); if ((r = hb_upload(c, 4, (const int *)a.data(), a.size(), &hb.j3_same))) return r; }
  { auto a = hb_transpose3(t->J_three_orbital_probabilities_opposite_spin, n); if ((r = hb_upload(c, 5, (const int *)a.data(), a.size(), &hb.j3_opp))) return r; }
  { auto a = hb_transpose3(t->q_three_orbital_probabilities_same_spin, n); if ((r = hb_upload(c, 6, a.data(), a.size(), &hb.q3_same))) return r; }
  { auto a = hb_transpose3(t->q_three_orbital_probabilities_opposite_spin, n); if ((r = hb_upload(c, 7, a.data(), a.size(), &hb.q3_opp))) return r; }
  if ((r = hb_upload(c, 8, t->four_orbital_probabilities_same_spin, (size_t)t->size_same, &hb.four_same))) return r;
  if ((r = hb_upload(c, 9, t->four_orbital_probabilities_opposite_spin, (size_t)t->size_opposite, &hb.four_opp))) return r;
  if ((r = hb_upload(c, 10, (const int *)t->J_four_orbital_probabilities_same_spin, (size_t)t->size_same, &hb.j4_same))) return r;
  if ((r = hb_upload(c, 11, (const int *)t->J_four_orbital_probabilities_opposite_spin, (size_t)t->size_opposite, &hb.j4_opp))) return r;
  if ((r = hb_upload(c, 12, t->q_four_orbital_probabilities_same_spin, (size_t)t->size_same, &hb.q4_same))) return r;
  if ((r = hb_upload(c, 13, t->q_four_orbital_probabilities_opposite_spin, (size_t)t->size_opposite, &hb.q4_opp))) return r;
  { std::vector<double> a((size_t)npairs * n);          // (p,k) column-major -> [p][k]
    for (long long p = 0; p < npairs; p++) for (int k = 0; k < n; k++) a[(size_t)p * n + k] = t->Htot_same[(size_t)p + (size_t)npairs * k];
    if ((r = hb_upload(c, 14, a.data(), a.size(), &hb.htot_same))) return r; }
  { auto a = hb_transpose3(t->Htot_opposite, n); if ((r = hb_upload(c, 15, a.data(), a.size(), &hb.htot_opp))) return r; }
  hb.on = 1;
  c->dev.hb = hb;
  return SQMC_OK;
}

int sqmc_gpu_propose_heatbath_batch(sqmc_gpu_ctx *c, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                                    uint64_t *ju, uint64_t *jd, double *wj, int32_t *seeds_after) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (!c->dev.hb.on) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_set_heatbath_tables not called");
  return propose_batch(k_propose_heatbath_batch, "sqmc_gpu_propose_heatbath_batch", 2, c, n, tau, up, dn, seeds, ju, jd, wj, seeds_after);
}

// setup_orb_by_symm, chemistry.f90:2505-2523, with proposal_method = 'CauchySchwarz'
int sqmc_gpu_setup_cauchy_schwarz(sqmc_gpu_ctx *c, int32_t *n_clamped) {
  abandon_head(c);
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "the Cauchy-Schwarz proposal is a 'chem' proposal");
  if (c->dev.hb.on) return fail(SQMC_ERR_BAD_ARG, "the context already proposes by fast heat-bath");
  // the tables may change integrals that H depends on: nothing built from them may exist yet (system_setup_chem order)
  if (c->n_imp > 0 || c->d_prj_ptr || c->d_ct_up || c->psit_on || c->nwalk > 0 || c->d_hb_r)
    return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_setup_cauchy_schwarz must come before the projector, C(T), Psi_T, the HCI tables and the walkers");
  const ChemTab &t = c->htab;
  const int n = t.norb;
  std::vector<double> ints((size_t)c->n_ints + 1);
  HIPCHK(hipMemcpy(ints.data(), c->d_ints, ints.size() * sizeof(double), hipMemcpyDeviceToHost));
  auto idx = [&](int i, int j) { const long long a = t.c2[i * t.c2_stride + j]; return (size_t)((a * (a - 1)) / 2 + a); };    // integral_index(i,j,i,j)
  const double stop_below = (double)-1e-6f;           // the literal is default real (2514)
  for (int i = 1; i <= n; i++) for (int j = 1; j <= n; j++)
    if (ints[idx(i, j)] < stop_below) return fail(SQMC_ERR_BAD_ARG, "Negative integrals!");
  int nclamp = 0;
  std::vector<double> sq((size_t)n * n, 0.0), orb(n, 0.0), sym((size_t)SQ_MAXSYM * n, 0.0);
  for (int i = 1; i <= n; i++)
    for (int j = 1; j <= n; j++) {
      const int s1 = t.orbsym[j];
      double &v = ints[idx(i, j)];
      if (v < 0) { v = 0; nclamp++; }
      const double r = sqrt(v);
      sq[(size_t)(i - 1) * n + (j - 1)] = r;
      sym[(size_t)(s1 - 1) * n + (i - 1)] = sym[(size_t)(s1 - 1) * n + (i - 1)] + r;
      orb[i - 1] = orb[i - 1] + r;
    }
  // the new tables are complete on the device before the old ones go: a failure part way leaves the context as it was
  const std::vector<double> *src[3] = {&sq, &orb, &sym};
  double *fresh[3] = {nullptr, nullptr, nullptr};
  for (int q = 0; q < 3; q++) {
    if (hipMalloc(&fresh[q], src[q]->size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(fresh[q], src[q]->data(), src[q]->size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      for (int k = 0; k <= q; k++) hipFree(fresh[k]);
      return fail(SQMC_ERR_HIP, "sqmc_gpu_setup_cauchy_schwarz: table upload failed");
    }
  }
  if (nclamp && hipMemcpy(c->d_ints, ints.data(), ints.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    for (int k = 0; k < 3; k++) hipFree(fresh[k]);
    return fail(SQMC_ERR_HIP, "sqmc_gpu_setup_cauchy_schwarz: integral upload failed");
  }
  for (int q = 0; q < 3; q++) { hipFree(c->d_cs[q]); c->d_cs[q] = fresh[q]; }
  CsDev cs; memset(&cs, 0, sizeof(cs));
  cs.on = 1; cs.norb = n; cs.sq = c->d_cs[0]; cs.orb = c->d_cs[1]; cs.sym = c->d_cs[2];
  c->dev.cs = cs;
  if (n_clamped) *n_clamped = nclamp;
  return SQMC_OK;
}

int sqmc_gpu_propose_cauchy_schwarz_batch(sqmc_gpu_ctx *c, int64_t n, double tau, const uint64_t *up, const uint64_t *dn, const int32_t *seeds,
                                          uint64_t *ju, uint64_t *jd, double *wj, int32_t *seeds_after) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (!c->dev.cs.on) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_setup_cauchy_schwarz not called");
  return propose_batch(k_propose_cauchy_batch, "sqmc_gpu_propose_cauchy_schwarz_batch", 1, c, n, tau, up, dn, seeds, ju, jd, wj, seeds_after);
}

int sqmc_gpu_hci_connections(sqmc_gpu_ctx *c, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn, const double *coeffs, double eps,
                             int diag_mode, int64_t *out_n, uint64_t **out_up, uint64_t **out_dn, double **out_num, double **out_den) {
  return sqmc_gpu_hci_connections_slice(c, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, 0, 1, out_n, out_up, out_dn, out_num, out_den);
}

// keep_dev != null: the deduplicated connections stay on the device (ou, od, onum, oden; the caller frees them) together with the
// reference determinants (dru, drd), and nothing is copied to the host
// rec: the generator carries the get_new_diag_elem record of every connection and the dedup keeps the first of each run (orold, orpk
// of keep_dev; with host output: *out_old, *out_pqrs as four int32 per connection, zeros where there is no record)
struct HciDevOut {
  DevScratch mem; u64 *ou = nullptr, *od = nullptr; double *onum = nullptr, *oden = nullptr; long long U = 0; u64 *dru = nullptr, *drd = nullptr; double *orold = nullptr; unsigned *orpk = nullptr;
  explicit HciDevOut(hipStream_t st) : mem(st) {}
};
static void hci_unpack_records(const unsigned *pk, long long n, int32_t *pqrs) {
  for (long long k = 0; k < n; k++) { pqrs[4 * k] = pk[k] & 255u; pqrs[4 * k + 1] = (pk[k] >> 8) & 255u; pqrs[4 * k + 2] = (pk[k] >> 16) & 255u; pqrs[4 * k + 3] = pk[k] >> 24; }
}
// Sorted ranks of n determinants on the device: k_main_keys, then the radix sort on the context's key bits.  *skey: the ranks ascending;
// *perm: the position of each in the input order.  The two key buffers (*skey is one of them) and rowtot belong to `keys`, the rest
// of the sort's scratch to `work` (the same owner, or one the caller clears sooner).  hist holds RS_MAX_RADIX counts per tile of the sort,
// ceil(n / RS_TILE) tiles at most (scan_sort.h: hist[digit * ntiles + tile]); two of the callers used to allocate one tile more than that.
static int det_ranks_sorted(sqmc_gpu_ctx *c, const char *who, long long n, const u64 *d_up, const u64 *d_dn, DevScratch &keys, DevScratch &work,
                            u64 **skey, u32 **perm, u32 **rowtot = nullptr) {
  u64 *vk = keys.take<u64>(n), *vkalt = keys.take<u64>(n); u32 *rt = keys.take<u32>(RS_MAX_RADIX);
  u32 *vv = work.take<u32>(n), *vvalt = work.take<u32>(n), *hist = work.take<u32>((size_t)((n + RS_TILE - 1) / RS_TILE) * RS_MAX_RADIX);
  if (!keys.ok() || !work.ok()) return hip_fail(who, keys.ok() ? work.err() : keys.err());
  hipLaunchKernelGGL(k_main_keys, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, d_up, d_dn, vk, vv, n, 0);
  SortWork so; so.k_alt = vkalt; so.v_alt = vvalt; so.hist = hist; so.rowtot = rt; so.cap = n;
  *skey = vk; *perm = vv;
  device_radix_sort(*skey, *perm, n, c->key_bits, so, c->st);
  if (rowtot) *rowtot = rt;
  return SQMC_OK;
}
static int hci_connections_impl(sqmc_gpu_ctx *c, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn, const double *coeffs, double eps,
                                int diag_mode, int32_t slice, int32_t n_slices, int64_t *out_n, uint64_t **out_up, uint64_t **out_dn,
                                double **out_num, double **out_den, HciDevOut *keep_dev, bool rec = false, double **out_old = nullptr, int32_t **out_pqrs = nullptr) {
  if (!c || !out_n) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (rec && (c->htab.time_sym || c->htab.sys_type >= 2)) return fail(SQMC_ERR_UNSUPPORTED, "the diagonal-update record is a determinant-basis formula for chem and heg contexts without time_sym");
  if (keep_dev && diag_mode == 2) return fail(SQMC_ERR_BAD_ARG, "raw mode has no device-resident form");
  if (n_slices < 1 || slice < 0 || slice >= n_slices) return fail(SQMC_ERR_BAD_ARG, "slice out of range");
  u64 key_lo = 0, key_hi = ~0ull;
  if (n_slices > 1) {                 // equal parts of the key range [0, invalid_key]
    const long double span = ((long double)c->invalid_key + 1.0L) / (long double)n_slices;
    key_lo = (u64)(span * slice); key_hi = (slice == n_slices - 1) ? (~0ull - 1ull) : (u64)(span * (slice + 1));
  }
  if (c->htab.sys_type == 0 && !c->dev.hb_r) return fail(SQMC_ERR_BAD_ARG, "heat-bath tables not set (sqmc_gpu_set_hb_tables)");
  if (c->htab.sys_type == 1 && c->htab.heg_nmax > 4) return fail(SQMC_ERR_UNSUPPORTED, "HEG connections: plane-wave index beyond +-4");
  *out_n = 0;
  if (n_ref <= 0) return SQMC_OK;
  const char *who = "sqmc_gpu_hci_connections";
  hipStream_t st = c->st;
  DevScratch s(st);
  const long long tiles = (n_ref + SCAN_TILE - 1) / SCAN_TILE + 1;
  u64 *dru = s.take<u64>(n_ref), *drd = s.take<u64>(n_ref); double *dco = s.take<double>(n_ref);
  u64 *dcnt = s.take<u64>(n_ref), *doff = s.take<u64>(n_ref), *dtot = s.take<u64>(1), *dts = s.take<u64>(tiles + 1);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemcpy(dru, ref_up, n_ref * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(drd, ref_dn, n_ref * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dco, coeffs, n_ref * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_hci_gen<false>, dim3(nblk(n_ref)), dim3(TPB), 0, st, c->dev, dru, drd, dco, eps, diag_mode, (long long)n_ref, 0, dcnt, doff,
                     (u64 *)nullptr, (u64 *)nullptr, (double *)nullptr, (double *)nullptr, key_lo, key_hi, c->as, (double *)nullptr, (unsigned *)nullptr);
  ScanWork sw = scan_work(dts, tiles);
  device_excl_scan_u64(dcnt, doff, n_ref, dtot, sw, st);
  u64 total = 0;
  HIPCHK(hipMemcpyAsync(&total, dtot, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  if (total == 0) return SQMC_OK;
  if (total >= (1ull << 31)) return fail(SQMC_ERR_UNSUPPORTED, "more than 2^31 connections in one call: use more slices (sqmc_gpu_hci_connections_slice)");
  const long long T = (long long)total;
  u64 *du = s.take<u64>(T), *dd = s.take<u64>(T); double *dnum = s.take<double>(T), *dden = s.take<double>(T);
  double *drold = rec ? s.take<double>(T) : nullptr; unsigned *drpk = rec ? s.take<unsigned>(T) : nullptr;
  if (!s.ok()) return hip_fail(who, s.err());
  hipLaunchKernelGGL(rec ? k_hci_gen<true> : k_hci_gen<false>, dim3(nblk(n_ref)), dim3(TPB), 0, st, c->dev, dru, drd, dco, eps, diag_mode, (long long)n_ref, 1, dcnt, doff,
                     du, dd, dnum, dden, key_lo, key_hi, c->as, drold, drpk);      // without records both are null
  HostOut h;
  // n connections from the device to fresh host arrays, with the records if the call carries them; the caller's pointers are written last
  auto to_host = [&](long long n, const u64 *xu, const u64 *xd, const double *xnum, const double *xden, const double *xold, const unsigned *xpk) -> int {
    uint64_t *hu = h.take<uint64_t>(n), *hd = h.take<uint64_t>(n); double *hn = h.take<double>(n), *hden = h.take<double>(n);
    HIPCHK(hipMemcpy(hu, xu, n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(hd, xd, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hn, xnum, n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(hden, xden, n * 8, hipMemcpyDeviceToHost));
    double *ho = nullptr; int32_t *hp = nullptr;
    if (rec) {
      ho = h.take<double>(n); hp = h.take<int32_t>(4 * n + 2); std::vector<unsigned> pk(n);
      HIPCHK(hipMemcpy(ho, xold, n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(pk.data(), xpk, n * 4, hipMemcpyDeviceToHost));
      hci_unpack_records(pk.data(), n, hp);
    }
    *out_n = n;
    h.commit(hu, out_up); h.commit(hd, out_dn); h.commit(hn, out_num); h.commit(hden, out_den); h.commit(ho, out_old); h.commit(hp, out_pqrs);
    return SQMC_OK;
  };
  if (diag_mode == 2) {               // the unmerged list, in generation order
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
    return to_host(T, du, dd, dnum, dden, drold, drpk);
  }
  u64 *skey; u32 *perm;
  { const int rs = det_ranks_sorted(c, who, T, du, dd, s, s, &skey, &perm); if (rs) return rs; }
  const long long tiles2 = (T + SCAN_TILE - 1) / SCAN_TILE + 1;
  u64 *flags = s.take<u64>(T), *pos = s.take<u64>(T), *dts2 = s.take<u64>(tiles2 + 1), *dtot2 = s.take<u64>(1);
  if (!s.ok()) return hip_fail(who, s.err());
  hipLaunchKernelGGL(k_hci_heads, dim3(nblk(T)), dim3(TPB), 0, st, skey, flags, T);
  ScanWork sw2 = scan_work(dts2, tiles2);
  device_excl_scan_u64(flags, pos, T, dtot2, sw2, st);
  u64 nuniq = 0;
  HIPCHK(hipMemcpyAsync(&nuniq, dtot2, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  const long long U = (long long)nuniq;
  DevScratch &o = keep_dev ? keep_dev->mem : s;      // the deduplicated arrays: the caller's when they stay on the device
  u64 *ou = o.take<u64>(U), *od = o.take<u64>(U); double *onum = o.take<double>(U), *oden = o.take<double>(U);
  double *orold = rec ? o.take<double>(U) : nullptr; unsigned *orpk = rec ? o.take<unsigned>(U) : nullptr;
  if (!o.ok()) return hip_fail(who, o.err());
  hipLaunchKernelGGL(rec ? k_hci_dedup<true> : k_hci_dedup<false>, dim3(nblk(T)), dim3(TPB), 0, st, skey, perm, flags, pos, du, dd, dnum, dden, ou, od, onum, oden, T,
                     (const double *)drold, (const unsigned *)drpk, orold, orpk);
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
  s.drop(drold); s.drop(drpk);
  if (!keep_dev) return to_host(U, ou, od, onum, oden, orold, orpk);
  s.keep(dru, o); s.keep(drd, o);
  keep_dev->ou = ou; keep_dev->od = od; keep_dev->onum = onum; keep_dev->oden = oden; keep_dev->U = U; keep_dev->dru = dru; keep_dev->drd = drd;
  keep_dev->orold = orold; keep_dev->orpk = orpk;
  *out_n = U;
  return SQMC_OK;
}

// core / virtual masks for the generator (hci.f90:150-182 builds them from n_var_e_up/dn and n_var_orbs; passed down to
// find_important_connected_dets_chem through get_next_det_list, second_order_pt and do_pt): state of the context until changed
int sqmc_gpu_hci_set_active_space(sqmc_gpu_ctx *c, uint64_t core_up, uint64_t core_dn, uint64_t virt_up, uint64_t virt_dn, int32_t mode) {
  if (!c || mode < 0 || mode > 2) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (mode && c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "active-space masks: chemistry only");
  c->as.mode = mode; c->as.core_up = core_up; c->as.core_dn = core_dn; c->as.virt_up = virt_up; c->as.virt_dn = virt_dn;
  return SQMC_OK;
}
int sqmc_gpu_hci_connections_slice(sqmc_gpu_ctx *c, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn, const double *coeffs, double eps,
                                   int diag_mode, int32_t slice, int32_t n_slices, int64_t *out_n, uint64_t **out_up, uint64_t **out_dn,
                                   double **out_num, double **out_den) {
  return hci_connections_impl(c, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, slice, n_slices, out_n, out_up, out_dn, out_num, out_den, nullptr);
}

// ----------------------------------------------------------------------- the O(N) diagonal update (diag_update.h)
int sqmc_gpu_diag_update_batch(sqmc_gpu_ctx *c, int64_t n, const double *old_diag, const int32_t *pqrs, const uint64_t *new_up, const uint64_t *new_dn,
                               int32_t form, double *new_diag) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (c->htab.sys_type == 2) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_diag_update_batch: hubbard2 has no diagonal update (its H_ii is U times the number of doubly occupied sites)");
  if (c->htab.sys_type == 3) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_diag_update_batch: hubbardk has no diagonal update (its H_ii is a sum of nup + ndn orbital energies)");
  if (c->htab.time_sym) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_diag_update_batch: a determinant-basis formula; run PT2 in the determinant basis on a context with time_sym = 0");
  if (form != 0 && form != 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_diag_update_batch: form must be 0 (one lane, reference order) or 1 (lane group)");
  if (n <= 0) return SQMC_OK;
  if (!old_diag || !pqrs || !new_up || !new_dn || !new_diag) return fail(SQMC_ERR_BAD_ARG, "null argument");
  DevScratch s(c->st);
  double *dold = s.take<double>(n), *dout = s.take<double>(n); int *dpq = s.take<int>(4 * n); u64 *du = s.take<u64>(n), *dd = s.take<u64>(n);
  int *dbad = s.take<int>(1);
  if (!s.ok()) return hip_fail("sqmc_gpu_diag_update_batch", s.err());
  HIPCHK(hipMemcpy(dold, old_diag, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dpq, pqrs, n * 16, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(du, new_up, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dd, new_dn, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(dbad, 0, 4, c->st));
  if (form == 0) hipLaunchKernelGGL(k_diag_update_batch<0>, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, (const double *)dold, (const int *)dpq, (const u64 *)du, (const u64 *)dd, dout, (long long)n, dbad);
  else hipLaunchKernelGGL(k_diag_update_batch<1>, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, (const double *)dold, (const int *)dpq, (const u64 *)du, (const u64 *)dd, dout, (long long)n, dbad);
  HIPCHK(hipGetLastError());
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, c->st)); HIPCHK(hipStreamSynchronize(c->st));      // the one status read
  if (!bad) HIPCHK(hipMemcpy(new_diag, dout, n * 8, hipMemcpyDeviceToHost));
  if (bad) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_diag_update_batch: a record does not describe a double excitation into its determinant (orbital out of 1..2 norb, "
                                         "p or q still occupied, r or s empty, spins of p/r or q/s differ, or wrong electron numbers); nothing was evaluated for it");
  return SQMC_OK;
}
int sqmc_gpu_hci_set_diag_update(sqmc_gpu_ctx *c, int32_t mode) {
  if (!c || mode < 0 || mode > 2) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_set_diag_update: mode must be 0, 1 or 2");
  if (mode && (c->htab.time_sym || c->htab.sys_type >= 2)) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_set_diag_update: chem and heg contexts without time_sym only");
  c->du_mode = mode;
  return SQMC_OK;
}
// milliseconds the term kernel of the last sqmc_gpu_hci_pt2 took, all slices (0 unless SQMC_PT2_TIME was set when the library loaded); not part of the ABI
int sqmc_gpu_debug_pt2_terms_ms(sqmc_gpu_ctx *c, double *ms) { if (!c || !ms) return SQMC_ERR_BAD_ARG; *ms = c->pt2_terms_ms; return SQMC_OK; }
// Test door of the bucket-boundary blocks (bucket_partition.h): k_bucket_boundaries on the context's stream over the caller's sorted keys.
int sqmc_gpu_debug_bucket_boundaries(sqmc_gpu_ctx *c, int64_t n0, const uint32_t *keys, int32_t B, const uint32_t *kb, const uint32_t *hint, const uint32_t *kb_prev,
                                     const uint32_t *pos_prev, const uint32_t *scount, uint32_t *pos, uint32_t *kb_out, uint32_t *hint_out) {
  if (!c || !keys || n0 < 1 || n0 >= (1ll << 31) || B < 1 || B > BK_MAXB) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_debug_bucket_boundaries: bad argument");
  if ((kb != nullptr) != (pos != nullptr)) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_debug_bucket_boundaries: kb and pos go together");
  if (hint_out && !kb_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_debug_bucket_boundaries: hint_out without kb_out");
  if (kb_out && (!scount || B > BK_REBAL_MAXB)) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_debug_bucket_boundaries: next boundaries need scount and B <= BK_REBAL_MAXB");
  for (int64_t i = 1; i < n0; i++) if (keys[i] < keys[i - 1]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_debug_bucket_boundaries: keys are not ascending");
  if (!kb && !kb_out) return SQMC_OK;
  const size_t nb = (size_t)B + 1;
  std::vector<u64> words(n0);
  for (int64_t i = 0; i < n0; i++) words[i] = ((u64)keys[i] << 32) | (u64)i;
  const char *who = "sqmc_gpu_debug_bucket_boundaries";
  DevScratch s(c->st);
  u64 *d_keys = s.take<u64>(n0); u32 *d_w = s.take<u32>(8 * nb);      // eight arrays of B + 1 words: kb, hint, kb_prev, pos_prev, scount, pos, kb_out, hint_out
  if (!s.ok()) return fail(SQMC_ERR_HIP, "hipMalloc");
  const uint32_t *in[5] = {kb, hint, kb_prev, pos_prev, scount};
  HIPDOOR(who, hipMemcpy(d_keys, words.data(), (size_t)n0 * 8, hipMemcpyHostToDevice));
  HIPDOOR(who, hipMemset(d_w, 0, 8 * nb * 4));
  for (int q = 0; q < 5; q++) if (in[q]) HIPDOOR(who, hipMemcpy(d_w + q * nb, in[q], nb * 4, hipMemcpyHostToDevice));
  BucketArgs ba; memset(&ba, 0, sizeof(ba));
  ba.B = B; ba.scount = d_w + 4 * nb;
  if (kb) { ba.kb = d_w; ba.pos = d_w + 5 * nb; if (hint) ba.hint = d_w + nb; }
  if (kb_prev) ba.kb_prev = d_w + 2 * nb;
  if (pos_prev) ba.pos_prev = d_w + 3 * nb;
  if (kb_out) { ba.kb_out = d_w + 6 * nb; if (hint_out) ba.hint_out = d_w + 7 * nb; }
  hipLaunchKernelGGL(k_bucket_boundaries, dim3(2), dim3(BK_T), 0, c->st, (const u64 *)d_keys, (long long)n0, ba);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, hipStreamSynchronize(c->st));
  if (pos) HIPDOOR(who, hipMemcpy(pos, d_w + 5 * nb, nb * 4, hipMemcpyDeviceToHost));
  if (kb_out) HIPDOOR(who, hipMemcpy(kb_out, d_w + 6 * nb, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (hint_out) HIPDOOR(who, hipMemcpy(hint_out, d_w + 7 * nb, (size_t)B * 4, hipMemcpyDeviceToHost));
  return SQMC_OK;
}
int sqmc_gpu_hci_connections_record(sqmc_gpu_ctx *c, int64_t n_ref, const uint64_t *ref_up, const uint64_t *ref_dn, const double *coeffs, double eps,
                                    int diag_mode, int32_t slice, int32_t n_slices, int64_t *out_n, uint64_t **out_up, uint64_t **out_dn,
                                    double **out_num, double **out_den, double **out_old_diag, int32_t **out_pqrs) {
  return hci_connections_impl(c, n_ref, ref_up, ref_dn, coeffs, eps, diag_mode, slice, n_slices, out_n, out_up, out_dn, out_num, out_den, nullptr, true, out_old_diag, out_pqrs);
}

// Deterministic Epstein-Nesbet second-order correction, second_order_pt (hci.f90:1100-1182):
//   delta_E = sum over the determinants a connected to the variational wavefunction but outside it of
//             (sum_i H_ai c_i)^2 / (E_var - H_aa),          the inner sum screened by |H_ai c_i| >= eps_pt,
// entirely on the device: connection generation + dedup-sum (the HCI generator), membership in the variational space by binary
// search on sorted determinant ranks (binary_search at hci.f90:1159), H_aa, and one fixed-shape reduction (the same value run to
// run).  n_slices > 1 cuts the connected space into that many parts of the determinant-rank range (exact: every connected
// determinant lives in one part) for spaces whose connections do not fit the card at once.
int sqmc_gpu_hci_pt2(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var, double eps_pt,
                     int32_t n_slices, double *delta_e, int64_t *n_connections) {
  if (!c || !delta_e || !n_connections || n_var <= 0 || n_slices < 1) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (c->htab.sys_type == 3 && c->htab.hk_sym) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2 is not built for hubbardk with space_sym");
  hipStream_t st = c->st;
  static const bool timed = getenv("SQMC_PT2_TIME") != nullptr;      // tools/pt2_diag_time.py: HIP events around the term kernel (membership + H_aa + term)
  c->pt2_terms_ms = 0.0;
  double total = 0.0; long long nconn = 0;
  // sorted ranks of the variational determinants
  const char *who = "sqmc_gpu_hci_pt2";
  DevScratch s(st);
  u64 *vu = s.take<u64>(n_var), *vd = s.take<u64>(n_var);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemcpy(vu, var_up, n_var * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(vd, var_dn, n_var * 8, hipMemcpyHostToDevice));
  u64 *skey; u32 *sperm;
  { const int rs = det_ranks_sorted(c, who, n_var, vu, vd, s, s, &skey, &sperm); if (rs) return rs; }
  EventMarks ev(timed, 2);
  for (int sl = 0; sl < n_slices; sl++) {
    HciDevOut d(st); int64_t U = 0;
    const int rc = hci_connections_impl(c, n_var, var_up, var_dn, coeffs, eps_pt, 0, sl, n_slices, &U, nullptr, nullptr, nullptr, nullptr, &d, c->du_mode != 0);
    if (rc != SQMC_OK) return rc;
    if (U > 0 && d.ou) {
      const int nb = std::min(nblk(U), 4096);
      double *dpart = d.mem.take<double>(nb);
      if (!d.mem.ok()) return hip_fail(who, d.mem.err());
      HIPCHK(ev.mark(st));
      if (c->du_mode)
        hipLaunchKernelGGL(c->du_mode == 1 ? k_pt2_terms_upd<0> : k_pt2_terms_upd<1>, dim3(nb), dim3(TPB), 0, st, c->dev, (const u64 *)d.ou, (const u64 *)d.od,
                           (const double *)d.onum, (const double *)d.orold, (const unsigned *)d.orpk, (long long)U, (const u64 *)skey, (long long)n_var, e_var, dpart);
      else
        hipLaunchKernelGGL(k_pt2_terms, dim3(nb), dim3(TPB), 0, st, c->dev, (const u64 *)d.ou, (const u64 *)d.od, (const double *)d.onum, (long long)U,
                           (const u64 *)skey, (long long)n_var, e_var, dpart);
      HIPCHK(ev.mark(st));
      std::vector<double> part(nb);
      HIPCHK(hipMemcpyAsync(part.data(), dpart, nb * 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
      ev.add(&c->pt2_terms_ms);
      double ssum = 0.0; for (int q = 0; q < nb; q++) ssum += part[q];          // block partials in block order
      total += ssum; nconn += U;
    }
  }
  *delta_e = total; *n_connections = nconn;
  return SQMC_OK;
}

// ----------------------------------------------------------------------- semistochastic PT2
// One sample of second_order_pt_alias (hci.f90:1314-1660) on the device.  The plan keeps the variational wavefunction, its sorted
// ranks and every work buffer; a sample allocates only when its raw connection count exceeds the capacity (n_alloc counts those
// events, the first included).
#define PT2S_MAXBLK 1024             // blocks of k_pt2s_terms at most (its partials are added by one wavefront)
struct sqmc_pt2s_plan {
  sqmc_gpu_ctx *c; long long n_var; int n_mc; double e_var, eps_pt, eps_pt_big;
  std::vector<double> prob;          // p_i = |c_i| / sum |c|
  u64 *vu, *vd, *skey; double *vc;                                    // variational determinants, coefficients, sorted ranks
  char *h_in; u64 *h_out;                                             // pinned: a sample's (w/p, ids) on the way in; total / (sum, count) on the way out
  char *d_in; u64 *d_ru, *d_rd, *d_cnt, *d_off, *d_tot, *d_scan, *d_out; double *d_rc; long long scan_tiles;
  long long cap; u64 *du, *dd, *keys, *kalt; double *dx, *dsrc; u32 *vals, *valt, *hist, *rowtot;     // per connection, capacity cap
  double *d_part; u64 *d_pcnt;
  int du_mode; double *drold; unsigned *drpk;                         // sqmc_gpu_hci_set_diag_update as it stood at prepare; the records, capacity cap (null in mode 0)
  long long n_alloc, n_samples, last_raw, max_raw;
  DevScratch mem, conn;              // owners of the device buffers above: those of the plan's lifetime; those of capacity cap, replaced when a sample outgrows them
};
// sum of n doubles in the blocked pairwise order (leaves of at most 128 summed in 8 interleaved accumulators, halves split on a
// multiple of 8): error O(log n) ulp, and the order numpy's sum uses, so that p_i has the bits of the host path
static double pt2s_pairwise_sum(const double *a, long long n) {
  if (n < 8) { double r = 0.0; for (long long i = 0; i < n; i++) r += a[i]; return r; }
  if (n <= 128) {
    double r[8]; for (int k = 0; k < 8; k++) r[k] = a[k];
    long long i;
    for (i = 8; i < n - (n % 8); i += 8) for (int k = 0; k < 8; k++) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
  }
  long long n2 = n / 2; n2 -= n2 % 8;
  return pt2s_pairwise_sum(a, n2) + pt2s_pairwise_sum(a + n2, n - n2);
}
static void pt2s_free_conn(sqmc_pt2s_plan *p) {
  p->conn.clear();
  p->du = p->dd = p->keys = p->kalt = nullptr; p->dx = p->dsrc = p->drold = nullptr; p->vals = p->valt = p->hist = p->drpk = nullptr; p->cap = 0;
}
static int pt2s_grow(sqmc_pt2s_plan *p, long long need) {
  pt2s_free_conn(p);
  long long cap = need + need / 4 + 1024;
  if (cap > (1ll << 31) - 1) cap = (1ll << 31) - 1;
  DevScratch &s = p->conn;
  p->du = s.take<u64>(cap); p->dd = s.take<u64>(cap); p->dx = s.take<double>(cap); p->dsrc = s.take<double>(cap);
  p->keys = s.take<u64>(cap); p->kalt = s.take<u64>(cap); p->vals = s.take<u32>(cap); p->valt = s.take<u32>(cap);
  p->hist = s.take<u32>((size_t)RS_MAX_RADIX * ((cap + RS_TILE - 1) / RS_TILE + 1));
  if (p->du_mode) { p->drold = s.take<double>(cap); p->drpk = s.take<unsigned>(cap); }
  if (!s.ok()) { const hipError_t e = s.err(); pt2s_free_conn(p); return hip_fail("sqmc_gpu_hci_pt2_stochastic_sample", e); }
  p->cap = cap; p->n_alloc++;
  return SQMC_OK;
}
int sqmc_gpu_hci_pt2_stochastic_free(sqmc_pt2s_plan *p) {
  if (!p) return SQMC_OK;
  p->conn.clear(); p->mem.clear();   // these wait for the context's stream (the handle of prepare: the plan goes before its context, as the header says)
  if (p->h_in) hipHostFree(p->h_in);   // behind the owners: nothing queued can still read the pinned buffers
  if (p->h_out) hipHostFree(p->h_out);
  delete p;
  return SQMC_OK;
}
static int pt2s_prepare(sqmc_pt2s_plan *p, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs) {
  const char *who = "sqmc_gpu_hci_pt2_stochastic_prepare";
  sqmc_gpu_ctx *c = p->c; hipStream_t st = c->st; const long long n = p->n_var, m = p->n_mc;
  DevScratch &s = p->mem;
  p->vu = s.take<u64>(n); p->vd = s.take<u64>(n); p->vc = s.take<double>(n);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(hipMemcpy(p->vu, var_up, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(p->vd, var_dn, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->vc, coeffs, n * 8, hipMemcpyHostToDevice));
  {
    DevScratch work(st);             // the permutation and the histogram go before the sample buffers come
    u32 *sperm;
    const int rs = det_ranks_sorted(c, who, n, p->vu, p->vd, s, work, &p->skey, &sperm, &p->rowtot);
    if (rs) return rs;
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
  }
  HIPCHK(hipHostMalloc(&p->h_in, m * 12 + 16)); HIPCHK(hipHostMalloc(&p->h_out, 32));
  p->d_in = s.take<char>(m * 12 + 16); p->d_ru = s.take<u64>(m); p->d_rd = s.take<u64>(m); p->d_rc = s.take<double>(m);
  p->d_cnt = s.take<u64>(m); p->d_off = s.take<u64>(m); p->d_tot = s.take<u64>(1); p->d_out = s.take<u64>(2);
  p->scan_tiles = (m + SCAN_TILE - 1) / SCAN_TILE + 1;
  p->d_scan = s.take<u64>(p->scan_tiles + 1);
  p->d_part = s.take<double>(PT2S_MAXBLK); p->d_pcnt = s.take<u64>(PT2S_MAXBLK);
  if (!s.ok()) return hip_fail(who, s.err());
  return SQMC_OK;
}
int sqmc_gpu_hci_pt2_stochastic_prepare(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var,
                                        double eps_pt, double eps_pt_big, int32_t n_mc, sqmc_pt2s_plan **plan) {
  if (!c || !plan || !var_up || !var_dn || !coeffs || n_var <= 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  *plan = nullptr;
  if (n_mc < 2) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_prepare: n_mc must be at least 2 (the estimator divides by n_mc (n_mc - 1))");
  if (n_var >= (1ll << 31)) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2_stochastic_prepare: more than 2^31 variational determinants");
  if (c->htab.sys_type == 2) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2_stochastic_prepare: the stochastic PT plan is not built for hubbard2");
  if (c->htab.sys_type == 3) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2_stochastic_prepare: the stochastic PT plan is not built for hubbardk");
  // Raw mode keeps the two raw excitations that take one source to one time-reversal representative apart: term2 would hold
  // x'^2 + x''^2 where the estimator needs (x' + x'')^2, and the big mask would see the element after the time-reversal factors.
  if (c->htab.time_sym)
    return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2_stochastic_prepare: the estimator is biased on time-reversal representatives; pass the determinant-basis "
                                      "expansion (convert_time_symmetrized_to_dets, hci.f90:4365-4564) on a context initialised with time_sym = 0");
  if (c->htab.sys_type == 0 && !c->dev.hb_r) return fail(SQMC_ERR_BAD_ARG, "heat-bath tables not set (sqmc_gpu_set_hb_tables)");
  if (c->htab.sys_type == 1 && c->htab.heg_nmax > 4) return fail(SQMC_ERR_UNSUPPORTED, "HEG connections: plane-wave index beyond +-4");
  for (long long i = 1; i < n_var; i++)
    if (var_up[i - 1] > var_up[i] || (var_up[i - 1] == var_up[i] && var_dn[i - 1] >= var_dn[i]))
      return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_prepare: the variational determinants must be sorted by (up, dn) without repeats (hci.f90:1373-1380)");
  sqmc_pt2s_plan *p = new sqmc_pt2s_plan();       // value-initialised: every pointer null, every counter 0
  p->c = c; p->n_var = n_var; p->n_mc = n_mc; p->e_var = e_var; p->eps_pt = eps_pt; p->eps_pt_big = eps_pt_big; p->du_mode = c->du_mode;
  p->mem.stream = p->conn.stream = c->st;
  p->prob.resize(n_var);
  for (long long i = 0; i < n_var; i++) p->prob[i] = fabs(coeffs[i]);
  double norm = 0.0;                              // numpy adds the pairwise sums of consecutive 8192-element pieces left to right
  for (long long i = 0; i < n_var; i += 8192) { const double part = pt2s_pairwise_sum(p->prob.data() + i, std::min<long long>(8192, n_var - i)); norm = i ? norm + part : part; }
  if (!(norm > 0.0)) { delete p; return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_prepare: all coefficients are zero"); }
  for (long long i = 0; i < n_var; i++) p->prob[i] = p->prob[i] / norm;
  const int rc = pt2s_prepare(p, var_up, var_dn, coeffs);
  if (rc != SQMC_OK) { const std::string m = g_err; sqmc_gpu_hci_pt2_stochastic_free(p); return fail(rc, m); }
  *plan = p;
  return SQMC_OK;
}
int sqmc_gpu_hci_pt2_stochastic_sample(sqmc_pt2s_plan *p, int64_t n_distinct, const int64_t *ids, const int64_t *counts, double *value, int64_t *n_connected) {
  if (!p || !ids || !counts || !value || !n_connected) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (n_distinct < 1 || n_distinct > p->n_mc) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_sample: n_distinct must be in [1, n_mc]");
  sqmc_gpu_ctx *c = p->c; hipStream_t st = c->st; const long long m = n_distinct;
  double *h_wop = (double *)p->h_in; int *h_ids = (int *)(p->h_in + (size_t)p->n_mc * 8);
  for (long long i = 0; i < m; i++) {
    if (ids[i] < 0 || ids[i] >= p->n_var) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_sample: id out of range (0-based positions in the variational list)");
    if (i > 0 && ids[i] <= ids[i - 1]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_sample: ids must be ascending and distinct (sort_and_merge_count_repeats)");
    if (counts[i] < 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_pt2_stochastic_sample: a count below 1");
  }
  for (long long i = 0; i < m; i++) { h_ids[i] = (int)ids[i]; h_wop[i] = (double)counts[i] / p->prob[ids[i]]; }
  const double *d_wop = (const double *)p->d_in; const int *d_ids = (const int *)(p->d_in + (size_t)p->n_mc * 8);
  HIPCHK(hipMemcpyAsync(p->d_in, p->h_in, (size_t)p->n_mc * 8 + m * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pt2s_gather, dim3(nblk(m)), dim3(TPB), 0, st, d_ids, (const u64 *)p->vu, (const u64 *)p->vd, (const double *)p->vc, p->d_ru, p->d_rd, p->d_rc, m);
  hipLaunchKernelGGL(k_hci_gen<false>, dim3(nblk(m)), dim3(TPB), 0, st, c->dev, p->d_ru, p->d_rd, p->d_rc, p->eps_pt, 2, m, 0, p->d_cnt, p->d_off,
                     (u64 *)nullptr, (u64 *)nullptr, (double *)nullptr, (double *)nullptr, 0ull, ~0ull, c->as, (double *)nullptr, (unsigned *)nullptr);
  ScanWork sw; sw.state = p->d_scan; sw.ticket = (u32 *)(p->d_scan + p->scan_tiles); sw.cap_tiles = p->scan_tiles; sw.self_clear = true;
  device_excl_scan_u64(p->d_cnt, p->d_off, m, p->d_tot, sw, st);
  HIPCHK(hipMemcpyAsync(p->h_out, p->d_tot, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));       // the one sync that sizes the fill
  const u64 total = p->h_out[0];
  if (total >= (1ull << 31)) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_hci_pt2_stochastic_sample: 2^31 or more raw connections in one sample (no slicing here: lower n_mc or raise eps_pt)");
  const long long T = (long long)total;
  p->last_raw = T; if (T > p->max_raw) p->max_raw = T;
  if (T == 0) { *value = 0.0; *n_connected = 0; p->n_samples++; return SQMC_OK; }
  if (T > p->cap) { const int rc = pt2s_grow(p, T); if (rc != SQMC_OK) return rc; }
  if (p->du_mode)
    hipLaunchKernelGGL(k_hci_gen<true>, dim3(nblk(m)), dim3(TPB), 0, st, c->dev, p->d_ru, p->d_rd, p->d_rc, p->eps_pt, 2, m, 1, p->d_cnt, p->d_off,
                       p->du, p->dd, p->dx, p->dsrc, 0ull, ~0ull, c->as, p->drold, p->drpk);
  else
    hipLaunchKernelGGL(k_hci_gen<false>, dim3(nblk(m)), dim3(TPB), 0, st, c->dev, p->d_ru, p->d_rd, p->d_rc, p->eps_pt, 2, m, 1, p->d_cnt, p->d_off,
                       p->du, p->dd, p->dx, p->dsrc, 0ull, ~0ull, c->as, (double *)nullptr, (unsigned *)nullptr);
  hipLaunchKernelGGL(k_main_keys, dim3(nblk(T)), dim3(TPB), 0, st, c->dev, p->du, p->dd, p->keys, p->vals, T, 0);
  SortWork so; so.k_alt = p->kalt; so.v_alt = p->valt; so.hist = p->hist; so.rowtot = p->rowtot; so.cap = p->cap;
  u64 *skey = p->keys; u32 *perm = p->vals;
  device_radix_sort(skey, perm, T, c->key_bits, so, st);
  const int nb = std::min(nblk(T), PT2S_MAXBLK);
  if (p->du_mode)
    hipLaunchKernelGGL(p->du_mode == 1 ? k_pt2s_terms_upd<0> : k_pt2s_terms_upd<1>, dim3(nb), dim3(TPB), 0, st, c->dev, (const u64 *)skey, (const u32 *)perm, (const u64 *)p->du, (const u64 *)p->dd,
                       (const double *)p->dx, (const double *)p->dsrc, (const double *)p->drold, (const unsigned *)p->drpk, d_wop, T, (const u64 *)p->skey, p->n_var,
                       p->e_var, p->eps_pt_big, (double)(p->n_mc - 1), p->d_part, p->d_pcnt);
  else
    hipLaunchKernelGGL(k_pt2s_terms, dim3(nb), dim3(TPB), 0, st, c->dev, (const u64 *)skey, (const u32 *)perm, (const u64 *)p->du, (const u64 *)p->dd,
                       (const double *)p->dx, (const double *)p->dsrc, d_wop, T, (const u64 *)p->skey, p->n_var, p->e_var, p->eps_pt_big,
                       (double)(p->n_mc - 1), p->d_part, p->d_pcnt);
  hipLaunchKernelGGL(k_pt2s_final, dim3(1), dim3(64), 0, st, (const double *)p->d_part, (const u64 *)p->d_pcnt, nb, p->d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(p->h_out + 2, p->d_out, 16, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  double sum; memcpy(&sum, &p->h_out[2], 8);
  *value = sum / ((double)p->n_mc * (double)(p->n_mc - 1));
  *n_connected = (int64_t)p->h_out[3];
  p->n_samples++;
  return SQMC_OK;
}
int sqmc_gpu_hci_pt2_stochastic_stats(sqmc_pt2s_plan *p, int64_t *n_alloc, int64_t *capacity, int64_t *last_raw, int64_t *n_samples) {
  if (!p) return fail(SQMC_ERR_BAD_ARG, "null plan");
  if (n_alloc) *n_alloc = p->n_alloc;
  if (capacity) *capacity = p->cap;
  if (last_raw) *last_raw = p->last_raw;
  if (n_samples) *n_samples = p->n_samples;
  return SQMC_OK;
}

// ----------------------------------------------------------------------- SpMV
int sqmc_gpu_spmv_prepare(int64_t n, const int64_t *rc, const int64_t *idx, const double *val, sqmc_spmv_plan **plan) {
  if (!rc || !idx || !val || !plan || n <= 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQMC_ERR_HIP, "no HIP device: libsqmc_gpu has no CPU fallback");
  long long nnz = 0; for (long long i = 0; i < n; i++) nnz += rc[i];
  for (long long k = 0; k < nnz; k++) if (idx[k] < 1 || idx[k] > n) return fail(SQMC_ERR_BAD_ARG, "column index out of range");
  if (2 * nnz >= (1ll << 31)) return fail(SQMC_ERR_UNSUPPORTED, "more than 2^31 expanded nonzeros");
  std::vector<int> ptr, col; std::vector<double> v;
  expand_full_csr(n, rc, idx, val, ptr, col, v);
  SpmvPlanOwned *p = nullptr;
  { const int rp = spmv_plan_new(n, (long long)col.size(), &p); if (rp) return rp; }
  std::unique_ptr<sqmc_spmv_plan, int (*)(sqmc_spmv_plan *)> guard(p, sqmc_gpu_spmv_free);
  HIPCHK(hipMemcpy(p->d_ptr, ptr.data(), (n + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(p->d_col, col.data(), col.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->d_val, v.data(), v.size() * 8, hipMemcpyHostToDevice));
  if (getenv("SQMC_SPMV_UPPER_ATOMIC")) {        // measurement only: the stored triangle + atomics (spmv_kernels.h)
    std::vector<int> up(n + 1, 0), uc(nnz);
    for (long long i = 0; i < n; i++) up[i + 1] = up[i] + (int)rc[i];
    for (long long k = 0; k < nnz; k++) uc[k] = (int)(idx[k] - 1);
    p->u_ptr = p->mem.take<int>(n + 1); p->u_col = p->mem.take<int>(nnz + 1); p->u_val = p->mem.take<double>(nnz + 1);
    if (!p->mem.ok()) return hip_fail("sqmc_gpu_spmv_prepare", p->mem.err());
    HIPCHK(hipMemcpy(p->u_ptr, up.data(), (n + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(p->u_col, uc.data(), nnz * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p->u_val, val, nnz * 8, hipMemcpyHostToDevice));
  }
  *plan = guard.release();
  return SQMC_OK;
}
int sqmc_gpu_spmv_apply(sqmc_spmv_plan *p, const double *x, double *y, int on_device) {
  if (!p || !x || !y) return fail(SQMC_ERR_BAD_ARG, "null");
  const double *dx = x; double *dy = y;
  if (!on_device) { HIPCHK(hipMemcpyAsync(p->d_x, x, p->n * 8, hipMemcpyHostToDevice, p->st)); dx = p->d_x; dy = p->d_y; }
  if (p->u_ptr && getenv("SQMC_SPMV_UPPER_ATOMIC")) {
    HIPCHK(hipMemsetAsync(dy, 0, p->n * 8, p->st));
    hipLaunchKernelGGL(k_spmv_upper_atomic, dim3((unsigned)((p->n + SPMV_ROWS_PER_BLOCK - 1) / SPMV_ROWS_PER_BLOCK)), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, p->st,
                       p->u_ptr, p->u_col, p->u_val, dx, dy, p->n);
  } else
  if (getenv("SQMC_SPMV_PROBE_NO_GATHER"))
    hipLaunchKernelGGL(k_spmv_wave<1>, dim3((unsigned)((p->n + SPMV_ROWS_PER_BLOCK - 1) / SPMV_ROWS_PER_BLOCK)), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, p->st,
                       p->d_ptr, p->d_col, p->d_val, dx, dy, p->n);
  else
  hipLaunchKernelGGL(k_spmv_wave<0>, dim3((unsigned)((p->n + SPMV_ROWS_PER_BLOCK - 1) / SPMV_ROWS_PER_BLOCK)), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, p->st,
                     p->d_ptr, p->d_col, p->d_val, dx, dy, p->n);
  HIPCHK(hipGetLastError());
  if (!on_device) { HIPCHK(hipMemcpyAsync(y, p->d_y, p->n * 8, hipMemcpyDeviceToHost, p->st)); }
  HIPCHK(hipStreamSynchronize(p->st));
  return SQMC_OK;
}
int sqmc_gpu_spmv_free(sqmc_spmv_plan *p) {
  if (!p) return SQMC_OK;
  SpmvPlanOwned *q = static_cast<SpmvPlanOwned *>(p);      // every plan is made by spmv_plan_new
  q->mem.clear(); hipStreamDestroy(q->st); delete q;
  return SQMC_OK;
}
// The principal submatrix dst(i, j) = src(sel[i], sel[j]) of a resident plan as a plan of its own (submatrix_kernels.h): mark, count,
// scan, fill on the source plan's stream.  Everything lives in `s` until the call has succeeded; only then does the new plan take its
// five arrays, so an early return frees what was taken and has written nothing.
static double g_submatrix_ms[2];      // SQMC_SUBMATRIX_TIME=1 (tools/extrap_time.py): the last call's mark + count + scan, and its fill, by HIP events
int sqmc_gpu_spmv_plan_submatrix(const sqmc_spmv_plan *src, int64_t m, const int64_t *sel, sqmc_spmv_plan **dst, int64_t *out_nnz_full) {
  const char *who = "sqmc_gpu_spmv_plan_submatrix";
  static const bool timed = getenv("SQMC_SUBMATRIX_TIME") != nullptr;
  if (!src || !sel || !dst || !out_nnz_full) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_spmv_plan_submatrix: null argument");
  if (m < 1 || m > src->n) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_spmv_plan_submatrix: m must lie in [1, n of the source plan]");
  if (src->u_ptr || getenv("SQMC_SPMV_UPPER_ATOMIC"))
    return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_spmv_plan_submatrix: the stored triangle of the SQMC_SPMV_UPPER_ATOMIC layout is not extracted");
  const long long n = src->n;
  hipStream_t st = src->st;
  DevScratch s(st);
  const long long tiles = (m + SCAN_TILE - 1) / SCAN_TILE + 1;
  long long *dsel = s.take<long long>(m); int *inv = s.take<int>(n);
  u64 *cnt = s.take<u64>(m), *off = s.take<u64>(m), *dtot = s.take<u64>(2), *dts = s.take<u64>(tiles + 1);      // dtot: the kept entries, the flag of a refused sel
  if (!s.ok()) return hip_fail(who, s.err());
  ScanWork sw = scan_work(dts, tiles);
  const unsigned wave_blocks = (unsigned)((m + SPMV_ROWS_PER_BLOCK - 1) / SPMV_ROWS_PER_BLOCK);
  HIPCHK(hipMemcpyAsync(dsel, sel, m * 8, hipMemcpyHostToDevice, st));
  EventMarks ev(timed, 2);
  g_submatrix_ms[0] = g_submatrix_ms[1] = 0.0;
  HIPCHK(ev.mark(st));
  HIPCHK(hipMemsetAsync(inv, 0xff, n * 4, st)); HIPCHK(hipMemsetAsync(dtot, 0, 16, st));
  hipLaunchKernelGGL(k_sub_mark, dim3(nblk(m)), dim3(TPB), 0, st, (const long long *)dsel, (long long)m, n, inv, dtot + 1);
  hipLaunchKernelGGL(k_sub_count, dim3(wave_blocks), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, st, (const int *)src->d_ptr, (const int *)src->d_col, (const long long *)dsel,
                     (const int *)inv, (const u64 *)(dtot + 1), cnt, (long long)m);
  device_excl_scan_u64(cnt, off, m, dtot, sw, st);
  u64 tot[2] = {0, 0};
  HIPCHK(hipGetLastError()); HIPCHK(ev.mark(st));
  HIPCHK(hipMemcpyAsync(tot, dtot, 16, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
  ev.add(&g_submatrix_ms[0]);
  if (tot[1]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_spmv_plan_submatrix: sel must be strictly ascending row numbers in [1, n] (1-based)");
  const long long nnz = (long long)tot[0];
  int *d_ptr = s.take<int>(m + 1), *d_col = s.take<int>(nnz + 1); double *d_val = s.take<double>(nnz + 1), *d_x = s.take<double>(m), *d_y = s.take<double>(m);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPCHK(ev.mark(st));
  hipLaunchKernelGGL(k_sub_fill, dim3(wave_blocks), dim3(64 * SPMV_ROWS_PER_BLOCK), 0, st, (const int *)src->d_ptr, (const int *)src->d_col, (const double *)src->d_val,
                     (const long long *)dsel, (const int *)inv, (const u64 *)off, d_ptr, d_col, d_val, (long long)m, nnz);
  HIPCHK(hipGetLastError()); HIPCHK(ev.mark(st)); HIPCHK(hipStreamSynchronize(st));
  ev.add(&g_submatrix_ms[1]);
  SpmvPlanOwned *p = new SpmvPlanOwned(); p->n = m; p->nnz_full = nnz;
  if (hipError_t e = hipStreamCreate(&p->st)) { delete p; return hip_fail(who, e); }
  p->mem.stream = p->st;
  p->d_ptr = d_ptr; p->d_col = d_col; p->d_val = d_val; p->d_x = d_x; p->d_y = d_y;
  s.keep(d_ptr, p->mem); s.keep(d_col, p->mem); s.keep(d_val, p->mem); s.keep(d_x, p->mem); s.keep(d_y, p->mem);
  *out_nnz_full = (int64_t)nnz; *dst = p;
  return SQMC_OK;
}
int sqmc_gpu_debug_submatrix_ms(double *count_ms, double *fill_ms) {      // not part of the ABI
  if (count_ms) *count_ms = g_submatrix_ms[0]; if (fill_ms) *fill_ms = g_submatrix_ms[1];
  return SQMC_OK;
}
// shell_sort_real_rank1_int_rank1 (host_sort.h): no device is touched
int sqmc_shell_sort_magnitude(int64_t n, double *a, int32_t *iorder) {
  if (n < 0 || (n > 0 && (!a || !iorder))) return fail(SQMC_ERR_BAD_ARG, "sqmc_shell_sort_magnitude: bad argument");
  host_shell_sort_magnitude(n, a, iorder);
  return SQMC_OK;
}
int sqmc_gpu_spmv_sym_upper(int64_t n, const int64_t *rc, const int64_t *idx, const double *val, const double *x, double *y) {
  sqmc_spmv_plan *p = nullptr;
  int r = sqmc_gpu_spmv_prepare(n, rc, idx, val, &p);
  if (r) return r;
  r = sqmc_gpu_spmv_apply(p, x, y, 0);
  sqmc_gpu_spmv_free(p);
  return r;
}

// ----------------------------------------------------------------------- the scratch owner's counters (dev_scratch.h); not part of the ABI
int sqmc_gpu_debug_scratch(int64_t *live_allocs, int64_t *live_bytes, int64_t *peak_bytes, int64_t *n_takes, int reset_peak) {
  if (live_allocs) *live_allocs = g_scratch_stats.live_allocs; if (live_bytes) *live_bytes = g_scratch_stats.live_bytes;
  if (peak_bytes) *peak_bytes = g_scratch_stats.peak_bytes; if (n_takes) *n_takes = g_scratch_stats.n_takes;       // peak: the most live_bytes has been since the last reset
  if (reset_peak) g_scratch_stats.peak_bytes = g_scratch_stats.live_bytes.load();
  return SQMC_OK;
}
// the nth take from now on fails without calling hipMalloc, once; 0 disarms
int sqmc_gpu_debug_scratch_fail_at(int64_t nth) { g_scratch_stats.fail_at = nth > 0 ? nth : 0; return SQMC_OK; }
