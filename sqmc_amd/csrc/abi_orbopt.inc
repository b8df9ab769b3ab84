// abi_orbopt.inc -- C-ABI entry point of the orbital gradient (inside extern "C"); kernels in orbopt_kernels.h, compiled in
// orbopt_device.hip and launched through orbopt_launch.h; the shape of the Fock GEMM in orbopt_plan.h.
// Textually included by sqmc_gpu.hip behind abi_rotate.inc (rot_check_combine2).

// tools/orbopt_time.py: HIP events around the kernels (SQMC_ORBOPT_TIME set when the library first runs the door)
static bool orbopt_timed() { static const bool on = getenv("SQMC_ORBOPT_TIME") != nullptr; return on; }

static int orbopt_door(sqmc_gpu_ctx *c, const double *one_rdm, const double *two_rdm_sf, double *fock_out, double *grad_out, double *hdiag_out) {
  const char *who = "sqmc_gpu_orbital_gradient";
  if (!c || !one_rdm || !two_rdm_sf) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbital_gradient: null argument");
  if (!fock_out && !grad_out && !hdiag_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbital_gradient: all three outputs are null");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_orbital_gradient: chem contexts only (heg, hubbard2 and hubbardk hold no integral table)");
  const ChemTab &t = c->htab;
  const int n = t.norb, n1 = n + 1, nn = n * n;
  const size_t n4 = (size_t)nn * nn;
  for (int e = 0; e < nn; e++) if (!std::isfinite(one_rdm[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbital_gradient: one_rdm holds a non-finite entry");
  for (size_t e = 0; e < n4; e++) if (!std::isfinite(two_rdm_sf[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbital_gradient: two_rdm_sf holds a non-finite entry");
  int rc = rot_check_combine2(c, who);
  if (rc != SQMC_OK) return rc;
  // 0-based pair table of the kernels, and the offset of the one-body block: integral_index(p, q, norb+1, norb+1) = A (A - 1) / 2 + combine_2(p, q)
  const long long A = t.c2[n1 * t.c2_stride + n1];
  const int hbase = (int)(A * (A - 1) / 2);
  std::vector<int> pair((size_t)nn);
  for (int p = 0; p < n; p++) for (int q = 0; q < n; q++) pair[(size_t)p * n + q] = t.c2[(p + 1) * t.c2_stride + (q + 1)];
  const OrbPlan plan = orbopt_plan(n);
  std::vector<double> host[3];           // declared ahead of s: s waits for the stream before a copy's target goes
  double *dst[3] = {fock_out, grad_out, hdiag_out};
  for (int k = 0; k < 3; k++) if (dst[k]) host[k].resize((size_t)nn);
  c->orbopt_ms[0] = c->orbopt_ms[1] = c->orbopt_ms[2] = 0.0;
  hipStream_t st = c->st;
  DevScratch s(st);
  double *d_D = s.take<double>(nn), *d_G = s.take<double>(n4); int *d_pair = s.take<int>(nn);
  double *d_part = s.take<double>((size_t)plan.nblocks * nn), *d_F = s.take<double>(nn);
  double *d_grad = grad_out ? s.take<double>(nn) : nullptr, *d_hd = hdiag_out ? s.take<double>(nn) : nullptr;
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpyAsync(d_D, one_rdm, (size_t)nn * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemcpyAsync(d_G, two_rdm_sf, n4 * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemcpyAsync(d_pair, pair.data(), (size_t)nn * sizeof(int), hipMemcpyHostToDevice, st));
  EventMarks ev(orbopt_timed(), 4);
  HIPDOOR(who, ev.mark(st));
  orbopt_launch_fock(st, plan, c->d_ints, d_pair, hbase, d_D, d_G, n, d_part, d_F);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st));
  if (d_grad) orbopt_launch_grad(st, d_F, n, d_grad);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st));
  if (d_hd) orbopt_launch_hdiag(st, c->d_ints, d_pair, hbase, d_D, d_G, d_F, n, d_hd);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st));
  const double *src[3] = {d_F, d_grad, d_hd};
  for (int k = 0; k < 3; k++) if (dst[k]) HIPDOOR(who, hipMemcpyAsync(host[k].data(), src[k], (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipStreamSynchronize(st));
  ev.add(c->orbopt_ms);
  for (int k = 0; k < 3; k++) if (dst[k]) memcpy(dst[k], host[k].data(), (size_t)nn * 8);      // only a finished call reaches the caller
  return SQMC_OK;
}
int sqmc_gpu_orbital_gradient(sqmc_gpu_ctx *c, const double *one_rdm, const double *two_rdm_sf, double *fock_out, double *grad_out, double *hdiag_out) {
  try { return orbopt_door(c, one_rdm, two_rdm_sf, fock_out, grad_out, hdiag_out); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_orbital_gradient: out of host memory"); }
}
// milliseconds the kernels of the last call took: the Fock GEMM with its reduction, the gradient, the diagonal Hessian (0 unless
// SQMC_ORBOPT_TIME was set when the library first ran the door); not part of the ABI
int sqmc_gpu_debug_orbopt_ms(sqmc_gpu_ctx *c, double *fock_ms, double *grad_ms, double *hdiag_ms) {
  if (!c || !fock_ms || !grad_ms || !hdiag_ms) return SQMC_ERR_BAD_ARG;
  *fock_ms = c->orbopt_ms[0]; *grad_ms = c->orbopt_ms[1]; *hdiag_ms = c->orbopt_ms[2];
  return SQMC_OK;
}
// the shape of the Fock GEMM at norb orbitals: register tile, triples per chunk, chunks per block, blocks; not part of the ABI
int sqmc_gpu_debug_orbopt_plan(int32_t norb, int64_t out[4]) {
  if (norb < 1 || norb > SQ_MAXORB || !out) return SQMC_ERR_BAD_ARG;
  const OrbPlan p = orbopt_plan(norb);
  out[0] = p.tm; out[1] = ORB_KC; out[2] = p.cpb; out[3] = p.nblocks;
  return SQMC_OK;
}
