// abi_greens.inc -- C-ABI entry point of the zeroth-order Green's function (inside extern "C"); kernels in greens_kernels.h
// Textually included by sqmc_gpu.hip behind abi_rdm.inc (RdmList, rdm_list_build); not a standalone file.

#define GF_PART_BYTES (64ull << 20)      // the chunk sums of one (list tile, frequency tile) stay below this (one chunk at least)

// tools/greens_time.py: HIP events around the two passes (SQMC_GREENS_TIME set when the library first runs one)
static bool gf_timed() { static const bool on = getenv("SQMC_GREENS_TIME") != nullptr; return on; }

// one half (N+1 or N-1) of a built list into d_g (n_w * norb * norb doubles on the device)
static int gf_half_dev(bool NP1, sqmc_gpu_ctx *c, const RdmList &L, double e0, int n_w, const double *d_w, int fermi, double *d_run, double *d_g) {
  const int norb = c->htab.norb, nup = c->htab.nup, ndn = c->htab.ndn;
  const int n_su = NP1 ? norb - nup : nup, nslot = n_su + (NP1 ? norb - ndn : ndn);
  const size_t nn = (size_t)norb * norb;
  hipStream_t st = c->st;
  HIPCHK(hipMemsetAsync(d_run, 0, (size_t)n_w * nn * 2 * 8, st));
  if (nslot == 0) { HIPCHK(hipMemsetAsync(d_g, 0, (size_t)n_w * nn * 8, st)); HIPCHK(hipStreamSynchronize(st)); return SQMC_OK; }
  const int wt_max = n_w < GF_WTILE ? n_w : GF_WTILE;
  const long long nchunks = (L.n + GF_CHUNK - 1) / GF_CHUNK;
  long long ctile = (long long)(GF_PART_BYTES / ((size_t)wt_max * nn * 2 * 8));
  if (ctile < 1) ctile = 1;
  if (ctile > nchunks) ctile = nchunks;
  const long long dtile = ctile * GF_CHUNK;
  const char *who = "sqmc_gpu_hci_greens_function";
  DevScratch s(st);
  double *poles = s.take<double>((size_t)(dtile < L.n ? dtile : L.n) * nslot), *part = s.take<double>((size_t)ctile * wt_max * nn * 2);
  if (!s.ok()) return hip_fail(who, s.err());
  EventMarks ev(gf_timed(), 3);
  for (long long j0 = 0; j0 < L.n; j0 += dtile) {
    const long long nd = (L.n - j0 < dtile) ? L.n - j0 : dtile;
    const int nch = (int)((nd + GF_CHUNK - 1) / GF_CHUNK);
    const int last = (j0 + dtile >= L.n) ? 1 : 0;
    HIPDOOR(who, ev.mark(st));
    if (NP1) hipLaunchKernelGGL(k_gf_poles<true>, dim3(nblk(nd * nslot)), dim3(TPB), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, j0, nd, n_su, nslot, e0, poles);
    else hipLaunchKernelGGL(k_gf_poles<false>, dim3(nblk(nd * nslot)), dim3(TPB), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, j0, nd, n_su, nslot, e0, poles);
    HIPDOOR(who, ev.mark(st));
    for (int w0 = 0; w0 < n_w; w0 += GF_WTILE) {
      const int wt = (n_w - w0 < GF_WTILE) ? n_w - w0 : GF_WTILE;
      if (NP1) hipLaunchKernelGGL(k_gf_terms<true>, dim3(nch, (unsigned)(nn * 2)), dim3(GF_T), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc,
                                  (const u64 *)L.skey, L.n, j0, nd, (const double *)poles, norb, n_su, nslot, fermi, d_w + w0, wt, part);
      else hipLaunchKernelGGL(k_gf_terms<false>, dim3(nch, (unsigned)(nn * 2)), dim3(GF_T), 0, st, c->dev, (const u64 *)L.su, (const u64 *)L.sd, (const double *)L.sc,
                              (const u64 *)L.skey, L.n, j0, nd, (const double *)poles, norb, n_su, nslot, fermi, d_w + w0, wt, part);
      hipLaunchKernelGGL(k_gf_sum, dim3(nblk((long long)wt * nn)), dim3(TPB), 0, st, (const double *)part, nch, norb, wt, w0, n_w, last, d_run, d_g);
    }
    HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st));
    HIPDOOR(who, hipStreamSynchronize(st));         // the next tile writes poles and part again
    ev.add(c->gf_ms);
  }
  return SQMC_OK;
}

int sqmc_gpu_hci_greens_function(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, double e0, int32_t n_w,
                                 const double *w, int32_t fermi_sign, double *g_np1, double *g_nm1) {
  const char *who = "sqmc_gpu_hci_greens_function";
  if (!c || !var_up || !var_dn || !coeffs || !w || n_var <= 0 || n_w <= 0) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": bad argument");
  if (!g_np1 && !g_nm1) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": both outputs are NULL");
  if (fermi_sign != 0 && fermi_sign != 1) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": fermi_sign must be 0 or 1");
  if (!std::isfinite(e0)) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": e0 is not finite");
  for (int i = 0; i < n_w; i++) if (!std::isfinite(w[i])) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": a frequency is not finite");
  if (c->htab.time_sym) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": a determinant-basis formula; pass the determinant-basis expansion to a context with time_sym = 0");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": the diagonal of the N+-1 electron determinants is hamiltonian_chem's; chem contexts only");
  if (!c->dev.integrals) return fail(SQMC_ERR_BAD_ARG, std::string(who) + ": the context holds no integrals");
  const int norb = c->htab.norb;
  const size_t nn = (size_t)norb * norb, ng = (size_t)n_w * nn;
  RdmList L(c->st);
  int rc = rdm_list_build(c, who, n_var, var_up, var_dn, coeffs, L);
  if (rc != SQMC_OK) return rc;
  c->gf_ms[0] = c->gf_ms[1] = 0.0;
  std::vector<double> host_p(g_np1 ? ng : 0), host_m(g_nm1 ? ng : 0);
  DevScratch s(c->st);
  double *d_w = s.take<double>(n_w), *d_run = s.take<double>(ng * 2), *d_g = s.take<double>(ng);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpy(d_w, w, (size_t)n_w * 8, hipMemcpyHostToDevice));
  if (g_np1) {
    if ((rc = gf_half_dev(true, c, L, e0, n_w, d_w, fermi_sign, d_run, d_g)) != SQMC_OK) return rc;
    if (hipMemcpy(host_p.data(), d_g, ng * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(SQMC_ERR_HIP, std::string(who) + ": copy back failed");
  }
  if (g_nm1) {
    if ((rc = gf_half_dev(false, c, L, e0, n_w, d_w, fermi_sign, d_run, d_g)) != SQMC_OK) return rc;
    if (hipMemcpy(host_m.data(), d_g, ng * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(SQMC_ERR_HIP, std::string(who) + ": copy back failed");
  }
  if (g_np1) memcpy(g_np1, host_p.data(), ng * 8);      // only finished arrays reach the caller
  if (g_nm1) memcpy(g_nm1, host_m.data(), ng * 8);
  return SQMC_OK;
}
// milliseconds the kernels of the last Green's function call took: the pole passes, the term passes (with their chunk sums), both halves
// added (0 unless SQMC_GREENS_TIME was set when the library first ran one); not part of the ABI
int sqmc_gpu_debug_greens_ms(sqmc_gpu_ctx *c, double *poles_ms, double *terms_ms) { if (!c || !poles_ms || !terms_ms) return SQMC_ERR_BAD_ARG; *poles_ms = c->gf_ms[0]; *terms_ms = c->gf_ms[1]; return SQMC_OK; }
