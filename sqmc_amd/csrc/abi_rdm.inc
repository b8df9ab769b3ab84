// abi_rdm.inc -- C-ABI entry points of the one-body reduced density matrix (inside extern "C"); kernels in rdm_kernels.h
// Textually included by sqmc_gpu.hip; not a standalone file.

// the determinant list of a 1-RDM call on the device, in rank order
struct RdmList { long long n; u64 *su, *sd, *skey; double *sc; void *mem[10]; int n_mem; };
static void rdm_list_free(RdmList &L) { for (int k = 0; k < L.n_mem; k++) hipFree(L.mem[k]); L.n_mem = 0; }
// checks, upload, ranks, sort, gather, repeats.  On any error everything allocated here is released.
static int rdm_list_build(sqmc_gpu_ctx *c, const char *who, int64_t n, const uint64_t *up, const uint64_t *dn, const double *coeffs, RdmList &L) {
  memset(&L, 0, sizeof(L));
  const std::string w(who);
  if (n >= (1ll << 31)) return fail(SQMC_ERR_UNSUPPORTED, w + ": more than 2^31 determinants");
  const u64 lim = c->htab.norb >= 64 ? ~0ull : ((1ull << c->htab.norb) - 1ull);
  for (long long i = 0; i < n; i++)
    if ((up[i] & ~lim) || (dn[i] & ~lim) || __builtin_popcountll(up[i]) != c->htab.nup || __builtin_popcountll(dn[i]) != c->htab.ndn)
      return fail(SQMC_ERR_BAD_ARG, w + ": a determinant does not hold nup / ndn electrons in the context's orbitals");
  hipStream_t st = c->st;
  u64 *vu, *vd, *vk, *vkalt, *su, *sd; u32 *vv, *vvalt, *hist, *rowtot; double *vc, *sc; int *flag;
  auto grab = [&](void **q, size_t bytes) -> bool { if (hipMalloc(q, bytes ? bytes : 8) != hipSuccess) { (void)hipGetLastError(); return false; } L.mem[L.n_mem++] = *q; return true; };
  u64 *tmp[4] = {nullptr, nullptr, nullptr, nullptr};      // released before returning: caller-order copies and sort scratch
  auto drop = [&]() { for (u64 *q : tmp) hipFree(q); };
  const size_t nt = (size_t)((n + RS_TILE - 1) / RS_TILE + 1);
  bool ok = grab((void **)&vk, n * 8) && grab((void **)&vkalt, n * 8) && grab((void **)&su, n * 8) && grab((void **)&sd, n * 8) && grab((void **)&sc, n * 8) &&
            grab((void **)&vv, n * 4) && grab((void **)&vvalt, n * 4) && grab((void **)&hist, nt * RS_MAX_RADIX * 4) && grab((void **)&rowtot, RS_MAX_RADIX * 4) && grab((void **)&flag, 4);
  ok = ok && hipMalloc(&tmp[0], n * 8) == hipSuccess && hipMalloc(&tmp[1], n * 8) == hipSuccess && hipMalloc(&tmp[2], n * 8) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); drop(); rdm_list_free(L); return fail(SQMC_ERR_HIP, w + ": hipMalloc failed"); }
  vu = tmp[0]; vd = tmp[1]; vc = (double *)tmp[2];
  hipError_t e = hipMemcpy(vu, up, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(vd, dn, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(vc, coeffs, n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(flag, 0, 4, st);
  int rep = 0;
  u64 *skey = vk; u32 *sperm = vv;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_main_keys, dim3(nblk(n)), dim3(TPB), 0, st, c->dev, vu, vd, vk, vv, (long long)n, 0);
    SortWork so; so.k_alt = vkalt; so.v_alt = vvalt; so.hist = hist; so.rowtot = rowtot; so.cap = n;
    device_radix_sort(skey, sperm, n, c->key_bits, so, st);
    hipLaunchKernelGGL(k_rdm_gather, dim3(nblk(n)), dim3(TPB), 0, st, (const u32 *)sperm, (const u64 *)vu, (const u64 *)vd, (const double *)vc, su, sd, sc, (long long)n);
    hipLaunchKernelGGL(k_rdm_repeats, dim3(nblk(n)), dim3(TPB), 0, st, (const u64 *)skey, (long long)n, flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&rep, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  drop();
  if (e != hipSuccess) { rdm_list_free(L); return fail(SQMC_ERR_HIP, w + ": " + hipGetErrorString(e)); }
  if (rep) { rdm_list_free(L); return fail(SQMC_ERR_BAD_ARG, w + ": a determinant appears twice in the list"); }
  L.n = n; L.su = su; L.sd = sd; L.sc = sc; L.skey = skey;
  return SQMC_OK;
}
// tools/rdm_time.py: HIP events around the kernels of a 1-RDM call (SQMC_RDM_TIME set when the library first runs one)
static bool rdm_timed() { static const bool on = getenv("SQMC_RDM_TIME") != nullptr; return on; }
static int rdm_refuse_basis(sqmc_gpu_ctx *c, const char *who) {
  if (c->htab.time_sym) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": a determinant-basis formula; pass the determinant-basis expansion to a context with time_sym = 0");
  if (c->htab.sys_type == 3 && c->htab.hk_sym) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + " is not built for hubbardk with space_sym");
  return SQMC_OK;
}
// the variational matrix of a built list into d_rdm (norb * norb doubles on the device); dsym: norb labels on the device or null
static int rdm_var_dev(sqmc_gpu_ctx *c, const RdmList &L, const unsigned char *dsym, double *d_rdm) {
  const int norb = c->htab.norb, nchunks = (int)((L.n + RDM_CHUNK - 1) / RDM_CHUNK);
  double *part; HIPCHK(hipMalloc(&part, (size_t)nchunks * norb * norb * 2 * 8));
  hipEvent_t ev[2]; const bool timed = rdm_timed();
  c->rdm_var_ms = 0.0;
  if (timed) { HIPCHK(hipEventCreate(&ev[0])); HIPCHK(hipEventCreate(&ev[1])); HIPCHK(hipEventRecord(ev[0], c->st)); }
  hipLaunchKernelGGL(k_rdm_terms<false>, dim3(nchunks, norb * norb * 2), dim3(RDM_T), 0, c->st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc, L.n,
                     (const u64 *)L.skey, (const double *)L.sc, L.n, norb, dsym, part);
  hipLaunchKernelGGL(k_rdm_sum, dim3(nblk(norb * norb)), dim3(TPB), 0, c->st, (const double *)part, nchunks, norb, d_rdm);
  hipError_t e = hipGetLastError();
  if (timed && e == hipSuccess) e = hipEventRecord(ev[1], c->st);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);
  if (timed) { float ms = 0.f; if (e == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->rdm_var_ms = ms; hipEventDestroy(ev[0]); hipEventDestroy(ev[1]); }
  hipFree(part);
  if (e != hipSuccess) return fail(SQMC_ERR_HIP, std::string("1-RDM kernels: ") + hipGetErrorString(e));
  return SQMC_OK;
}

int sqmc_gpu_hci_1rdm(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, const int32_t *orbital_symmetries, double *rdm) {
  if (!c || !var_up || !var_dn || !coeffs || !rdm || n_var <= 0) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm: bad argument");
  int rc = rdm_refuse_basis(c, "sqmc_gpu_hci_1rdm");
  if (rc != SQMC_OK) return rc;
  const int norb = c->htab.norb;
  std::vector<unsigned char> sym(norb);
  if (orbital_symmetries)
    for (int i = 0; i < norb; i++) {
      if (orbital_symmetries[i] < 0 || orbital_symmetries[i] > 255) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm: an orbital symmetry label outside 0..255");
      sym[i] = (unsigned char)orbital_symmetries[i];
    }
  RdmList L;
  rc = rdm_list_build(c, "sqmc_gpu_hci_1rdm", n_var, var_up, var_dn, coeffs, L);
  if (rc != SQMC_OK) return rc;
  double *d_rdm = nullptr; unsigned char *dsym = nullptr;
  std::vector<double> host((size_t)norb * norb);
  hipError_t e = hipMalloc(&d_rdm, (size_t)norb * norb * 8);
  if (e == hipSuccess && orbital_symmetries) { e = hipMalloc(&dsym, norb); if (e == hipSuccess) e = hipMemcpy(dsym, sym.data(), norb, hipMemcpyHostToDevice); }
  if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(SQMC_ERR_HIP, std::string("sqmc_gpu_hci_1rdm: ") + hipGetErrorString(e)); }
  if (rc == SQMC_OK) rc = rdm_var_dev(c, L, dsym, d_rdm);
  if (rc == SQMC_OK && hipMemcpy(host.data(), d_rdm, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(SQMC_ERR_HIP, "sqmc_gpu_hci_1rdm: copy back failed");
  hipFree(d_rdm); hipFree(dsym); rdm_list_free(L);
  if (rc != SQMC_OK) return rc;
  memcpy(rdm, host.data(), host.size() * 8);      // only a finished matrix reaches the caller
  return SQMC_OK;
}

int sqmc_gpu_hci_1rdm_pt(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var, double eps_pt_big,
                         int32_t n_slices, double *rdm, int64_t *n_connections) {
  if (!c || !var_up || !var_dn || !coeffs || !rdm || !n_connections || n_var <= 0 || n_slices < 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm_pt: bad argument");
  int rc = rdm_refuse_basis(c, "sqmc_gpu_hci_1rdm_pt");
  if (rc != SQMC_OK) return rc;
  if (c->htab.sys_type == 0 && !c->dev.hb_r) return fail(SQMC_ERR_BAD_ARG, "heat-bath tables not set (sqmc_gpu_set_hb_tables)");
  if (c->htab.sys_type == 1 && c->htab.heg_nmax > 4) return fail(SQMC_ERR_UNSUPPORTED, "HEG connections: plane-wave index beyond +-4");
  const int norb = c->htab.norb; hipStream_t st = c->st;
  RdmList L;
  rc = rdm_list_build(c, "sqmc_gpu_hci_1rdm_pt", n_var, var_up, var_dn, coeffs, L);
  if (rc != SQMC_OK) return rc;
  const int nchunks = (int)((L.n + RDM_CHUNK - 1) / RDM_CHUNK);
  const size_t nn = (size_t)norb * norb;
  c->rdm_pt_ms = 0.0;
  double *d_var = nullptr, *d_T = nullptr, *d_out = nullptr, *part = nullptr;
  std::vector<double> host(nn);
  long long nconn = 0;
  // the generator adds a connected determinant's terms in source order: hand it the list in rank order, so that the matrix has the
  // same bits for every order of the caller's list
  std::vector<u64> hu(n_var), hd(n_var); std::vector<double> hc(n_var);
  hipError_t e = hipMemcpy(hu.data(), L.su, n_var * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hd.data(), L.sd, n_var * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hc.data(), L.sc, n_var * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMalloc(&d_var, nn * 8);
  if (e == hipSuccess) e = hipMalloc(&d_T, nn * 8);
  if (e == hipSuccess) e = hipMalloc(&d_out, nn * 8);
  if (e == hipSuccess) e = hipMalloc(&part, (size_t)nchunks * nn * 2 * 8);
  if (e == hipSuccess) e = hipMemsetAsync(d_T, 0, nn * 8, st);
  if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(SQMC_ERR_HIP, std::string("sqmc_gpu_hci_1rdm_pt: ") + hipGetErrorString(e)); }
  if (rc == SQMC_OK) rc = rdm_var_dev(c, L, nullptr, d_var);
  for (int sl = 0; sl < n_slices && rc == SQMC_OK; sl++) {
    HciDevOut d; int64_t U = 0;
    rc = hci_connections_impl(c, n_var, (const uint64_t *)hu.data(), (const uint64_t *)hd.data(), hc.data(), eps_pt_big, 0, sl, n_slices, &U, nullptr, nullptr, nullptr, nullptr, &d);
    if (rc != SQMC_OK) break;
    if (U > 0 && d.ou) {
      u64 *ckey = nullptr; double *psi1 = nullptr;
      e = hipMalloc(&ckey, U * 8);
      if (e == hipSuccess) e = hipMalloc(&psi1, U * 8);
      hipEvent_t ev[2]; const bool timed = rdm_timed() && e == hipSuccess;
      if (timed) { hipEventCreate(&ev[0]); hipEventCreate(&ev[1]); hipEventRecord(ev[0], st); }
      if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rdm_psi1, dim3(nblk(U)), dim3(TPB), 0, st, c->dev, (const u64 *)d.ou, (const u64 *)d.od, (const double *)d.onum, (long long)U,
                           (const u64 *)L.skey, L.n, e_var, ckey, psi1);
        hipLaunchKernelGGL(k_rdm_terms<true>, dim3(nchunks, norb * norb * 2), dim3(RDM_T), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc, L.n,
                           (const u64 *)ckey, (const double *)psi1, (long long)U, norb, (const unsigned char *)nullptr, part);
        hipLaunchKernelGGL(k_rdm_pt_sum, dim3(nblk(norb * norb)), dim3(TPB), 0, st, (const double *)part, nchunks, norb, d_T);
        e = hipGetLastError();
        if (timed) hipEventRecord(ev[1], st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
      }
      if (timed) { float ms = 0.f; if (e == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->rdm_pt_ms += ms; hipEventDestroy(ev[0]); hipEventDestroy(ev[1]); }
      hipFree(ckey); hipFree(psi1);
      if (e != hipSuccess) { (void)hipGetLastError(); rc = fail(SQMC_ERR_HIP, std::string("sqmc_gpu_hci_1rdm_pt: ") + hipGetErrorString(e)); }
      nconn += U;
    }
    void *fr[] = {d.ou, d.od, d.onum, d.oden, d.dru, d.drd, d.orold, d.orpk};
    for (void *q : fr) hipFree(q);
  }
  if (rc == SQMC_OK) {
    hipLaunchKernelGGL(k_rdm_pt_final, dim3(nblk(norb * norb)), dim3(TPB), 0, st, (const double *)d_var, (const double *)d_T, norb, d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_out, nn * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = fail(SQMC_ERR_HIP, std::string("sqmc_gpu_hci_1rdm_pt: ") + hipGetErrorString(e));
  }
  hipFree(d_var); hipFree(d_T); hipFree(d_out); hipFree(part); rdm_list_free(L);
  if (rc != SQMC_OK) return rc;
  memcpy(rdm, host.data(), nn * 8);
  *n_connections = nconn;
  return SQMC_OK;
}
// milliseconds the kernels of the last 1-RDM call took: the variational pass, the PT passes of all slices (0 unless SQMC_RDM_TIME was set when the
// library first ran one); not part of the ABI
int sqmc_gpu_debug_rdm_ms(sqmc_gpu_ctx *c, double *var_ms, double *pt_ms) { if (!c || !var_ms || !pt_ms) return SQMC_ERR_BAD_ARG; *var_ms = c->rdm_var_ms; *pt_ms = c->rdm_pt_ms; return SQMC_OK; }
