// abi_rdm.inc -- C-ABI entry points of the one-body reduced density matrix (inside extern "C"); kernels in rdm_kernels.h
// Textually included by sqmc_gpu.hip; not a standalone file.

// the determinant list of a 1-RDM call on the device, in rank order; the list owns its buffers
struct RdmList { DevScratch mem; long long n = 0; u64 *su = nullptr, *sd = nullptr, *skey = nullptr; double *sc = nullptr, *sc2 = nullptr; explicit RdmList(hipStream_t st) : mem(st) {} };
// checks, upload, ranks, sort, gather, repeats.  coeffs2: a second coefficient array over the same list (the transition matrices' bra)
// or null; gathered by the same permutation into L.sc2
static int rdm_list_build(sqmc_gpu_ctx *c, const char *who, int64_t n, const uint64_t *up, const uint64_t *dn, const double *coeffs, RdmList &L, const double *coeffs2 = nullptr) {
  const std::string w(who);
  if (n >= (1ll << 31)) return fail(SQMC_ERR_UNSUPPORTED, w + ": more than 2^31 determinants");
  const u64 lim = c->htab.norb >= 64 ? ~0ull : ((1ull << c->htab.norb) - 1ull);
  for (long long i = 0; i < n; i++)
    if ((up[i] & ~lim) || (dn[i] & ~lim) || __builtin_popcountll(up[i]) != c->htab.nup || __builtin_popcountll(dn[i]) != c->htab.ndn)
      return fail(SQMC_ERR_BAD_ARG, w + ": a determinant does not hold nup / ndn electrons in the context's orbitals");
  hipStream_t st = c->st;
  DevScratch work(st);                 // released before returning: caller-order copies, sort scratch, the repeat flag
  u64 *vu = work.take<u64>(n), *vd = work.take<u64>(n); double *vc = work.take<double>(n); int *flag = work.take<int>(1);
  u64 *su = L.mem.take<u64>(n), *sd = L.mem.take<u64>(n); double *sc = L.mem.take<double>(n);
  double *vc2 = coeffs2 ? work.take<double>(n) : nullptr, *sc2 = coeffs2 ? L.mem.take<double>(n) : nullptr;
  if (!work.ok() || !L.mem.ok()) return hip_fail(who, work.ok() ? L.mem.err() : work.err());
  HIPDOOR(who, hipMemcpy(vu, up, n * 8, hipMemcpyHostToDevice)); HIPDOOR(who, hipMemcpy(vd, dn, n * 8, hipMemcpyHostToDevice));
  HIPDOOR(who, hipMemcpy(vc, coeffs, n * 8, hipMemcpyHostToDevice)); HIPDOOR(who, hipMemsetAsync(flag, 0, 4, st));
  if (coeffs2) HIPDOOR(who, hipMemcpy(vc2, coeffs2, n * 8, hipMemcpyHostToDevice));
  u64 *skey; u32 *sperm;
  { const int rs = det_ranks_sorted(c, who, n, vu, vd, L.mem, work, &skey, &sperm); if (rs) return rs; }
  hipLaunchKernelGGL(k_rdm_gather, dim3(nblk(n)), dim3(TPB), 0, st, (const u32 *)sperm, (const u64 *)vu, (const u64 *)vd, (const double *)vc, su, sd, sc, (long long)n);
  if (coeffs2) hipLaunchKernelGGL(k_rdm_gather, dim3(nblk(n)), dim3(TPB), 0, st, (const u32 *)sperm, (const u64 *)vu, (const u64 *)vd, (const double *)vc2, su, sd, sc2, (long long)n);
  hipLaunchKernelGGL(k_rdm_repeats, dim3(nblk(n)), dim3(TPB), 0, st, (const u64 *)skey, (long long)n, flag);
  int rep = 0;
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, hipMemcpyAsync(&rep, flag, 4, hipMemcpyDeviceToHost, st)); HIPDOOR(who, hipStreamSynchronize(st));
  if (rep) return fail(SQMC_ERR_BAD_ARG, w + ": a determinant appears twice in the list");
  L.n = n; L.su = su; L.sd = sd; L.sc = sc; L.sc2 = sc2; L.skey = skey;
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
  const char *who = "1-RDM kernels";
  const int norb = c->htab.norb, nchunks = (int)((L.n + RDM_CHUNK - 1) / RDM_CHUNK);
  DevScratch s(c->st);
  double *part = s.take<double>((size_t)nchunks * norb * norb * 2);
  if (!s.ok()) return hip_fail(who, s.err());
  EventMarks ev(rdm_timed(), 2);
  c->rdm_var_ms = 0.0;
  HIPDOOR(who, ev.mark(c->st));
  hipLaunchKernelGGL(k_rdm_terms<false>, dim3(nchunks, norb * norb * 2), dim3(RDM_T), 0, c->st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc, L.n,
                     (const u64 *)L.skey, (const double *)L.sc, L.n, norb, dsym, part);
  hipLaunchKernelGGL(k_rdm_sum, dim3(nblk(norb * norb)), dim3(TPB), 0, c->st, (const double *)part, nchunks, norb, d_rdm);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(c->st)); HIPDOOR(who, hipStreamSynchronize(c->st));
  ev.add(&c->rdm_var_ms);
  return SQMC_OK;
}

int sqmc_gpu_hci_1rdm(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, const int32_t *orbital_symmetries, double *rdm) {
  const char *who = "sqmc_gpu_hci_1rdm";
  if (!c || !var_up || !var_dn || !coeffs || !rdm || n_var <= 0) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm: bad argument");
  int rc = rdm_refuse_basis(c, who);
  if (rc != SQMC_OK) return rc;
  const int norb = c->htab.norb;
  std::vector<unsigned char> sym(norb);
  if (orbital_symmetries)
    for (int i = 0; i < norb; i++) {
      if (orbital_symmetries[i] < 0 || orbital_symmetries[i] > 255) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm: an orbital symmetry label outside 0..255");
      sym[i] = (unsigned char)orbital_symmetries[i];
    }
  RdmList L(c->st);
  if ((rc = rdm_list_build(c, who, n_var, var_up, var_dn, coeffs, L)) != SQMC_OK) return rc;
  DevScratch s(c->st);
  double *d_rdm = s.take<double>((size_t)norb * norb); unsigned char *dsym = orbital_symmetries ? s.take<unsigned char>(norb) : nullptr;
  if (!s.ok()) return hip_fail(who, s.err());
  if (dsym) HIPDOOR(who, hipMemcpy(dsym, sym.data(), norb, hipMemcpyHostToDevice));
  if ((rc = rdm_var_dev(c, L, dsym, d_rdm)) != SQMC_OK) return rc;
  std::vector<double> host((size_t)norb * norb);
  if (hipMemcpy(host.data(), d_rdm, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(SQMC_ERR_HIP, "sqmc_gpu_hci_1rdm: copy back failed");
  memcpy(rdm, host.data(), host.size() * 8);      // only a finished matrix reaches the caller
  return SQMC_OK;
}

int sqmc_gpu_hci_1rdm_pt(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e_var, double eps_pt_big,
                         int32_t n_slices, double *rdm, int64_t *n_connections) {
  const char *who = "sqmc_gpu_hci_1rdm_pt";
  if (!c || !var_up || !var_dn || !coeffs || !rdm || !n_connections || n_var <= 0 || n_slices < 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1rdm_pt: bad argument");
  int rc = rdm_refuse_basis(c, who);
  if (rc != SQMC_OK) return rc;
  if (c->htab.sys_type == 0 && !c->dev.hb_r) return fail(SQMC_ERR_BAD_ARG, "heat-bath tables not set (sqmc_gpu_set_hb_tables)");
  if (c->htab.sys_type == 1 && c->htab.heg_nmax > 4) return fail(SQMC_ERR_UNSUPPORTED, "HEG connections: plane-wave index beyond +-4");
  const int norb = c->htab.norb; hipStream_t st = c->st;
  RdmList L(st);
  if ((rc = rdm_list_build(c, who, n_var, var_up, var_dn, coeffs, L)) != SQMC_OK) return rc;
  const int nchunks = (int)((L.n + RDM_CHUNK - 1) / RDM_CHUNK);
  const size_t nn = (size_t)norb * norb;
  c->rdm_pt_ms = 0.0;
  long long nconn = 0;
  // the generator adds a connected determinant's terms in source order: hand it the list in rank order, so that the matrix has the
  // same bits for every order of the caller's list
  std::vector<u64> hu(n_var), hd(n_var); std::vector<double> hc(n_var);
  HIPDOOR(who, hipMemcpy(hu.data(), L.su, n_var * 8, hipMemcpyDeviceToHost)); HIPDOOR(who, hipMemcpy(hd.data(), L.sd, n_var * 8, hipMemcpyDeviceToHost));
  HIPDOOR(who, hipMemcpy(hc.data(), L.sc, n_var * 8, hipMemcpyDeviceToHost));
  std::vector<double> host(nn);          // declared ahead of s: s waits for the stream before the copy's target goes
  DevScratch s(st);
  double *d_var = s.take<double>(nn), *d_T = s.take<double>(nn), *d_out = s.take<double>(nn), *part = s.take<double>((size_t)nchunks * nn * 2);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemsetAsync(d_T, 0, nn * 8, st));
  if ((rc = rdm_var_dev(c, L, nullptr, d_var)) != SQMC_OK) return rc;
  EventMarks ev(rdm_timed(), 2);
  for (int sl = 0; sl < n_slices; sl++) {
    HciDevOut d(st); int64_t U = 0;
    rc = hci_connections_impl(c, n_var, (const uint64_t *)hu.data(), (const uint64_t *)hd.data(), hc.data(), eps_pt_big, 0, sl, n_slices, &U, nullptr, nullptr, nullptr, nullptr, &d);
    if (rc != SQMC_OK) return rc;
    if (U > 0 && d.ou) {
      u64 *ckey = d.mem.take<u64>(U); double *psi1 = d.mem.take<double>(U);
      if (!d.mem.ok()) return hip_fail(who, d.mem.err());
      HIPDOOR(who, ev.mark(st));
      hipLaunchKernelGGL(k_rdm_psi1, dim3(nblk(U)), dim3(TPB), 0, st, c->dev, (const u64 *)d.ou, (const u64 *)d.od, (const double *)d.onum, (long long)U,
                         (const u64 *)L.skey, L.n, e_var, ckey, psi1);
      hipLaunchKernelGGL(k_rdm_terms<true>, dim3(nchunks, norb * norb * 2), dim3(RDM_T), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc, L.n,
                         (const u64 *)ckey, (const double *)psi1, (long long)U, norb, (const unsigned char *)nullptr, part);
      hipLaunchKernelGGL(k_rdm_pt_sum, dim3(nblk(norb * norb)), dim3(TPB), 0, st, (const double *)part, nchunks, norb, d_T);
      HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st)); HIPDOOR(who, hipStreamSynchronize(st));
      ev.add(&c->rdm_pt_ms);
      nconn += U;
    }
  }
  hipLaunchKernelGGL(k_rdm_pt_final, dim3(nblk(norb * norb)), dim3(TPB), 0, st, (const double *)d_var, (const double *)d_T, norb, d_out);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, hipMemcpyAsync(host.data(), d_out, nn * 8, hipMemcpyDeviceToHost, st)); HIPDOOR(who, hipStreamSynchronize(st));
  memcpy(rdm, host.data(), nn * 8);      // only a finished matrix reaches the caller
  *n_connections = nconn;
  return SQMC_OK;
}
// milliseconds the kernels of the last 1-RDM call took: the variational pass, the PT passes of all slices (0 unless SQMC_RDM_TIME was set when the
// library first ran one); not part of the ABI
int sqmc_gpu_debug_rdm_ms(sqmc_gpu_ctx *c, double *var_ms, double *pt_ms) { if (!c || !var_ms || !pt_ms) return SQMC_ERR_BAD_ARG; *var_ms = c->rdm_var_ms; *pt_ms = c->rdm_pt_ms; return SQMC_OK; }
