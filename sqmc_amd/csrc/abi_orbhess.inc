// abi_orbhess.inc -- C-ABI entry points of the one-index transformation, of the resident orbital-optimisation plan and of the orbital
// Hessian-vector product (inside extern "C"); kernels in orbopt_kernels.h, compiled in orbopt_device.hip and launched through
// orbopt_launch.h; shapes in orbopt_plan.h.  Textually included by sqmc_gpu.hip behind abi_orbopt.inc.
//
//   sigma(kappa) = gradient formula (Fock GEMM on the one-index-transformed table; D, G)  +  1/2 (kappa g - g kappa)

// tools/orbhess_time.py: HIP events around the stages of a product (SQMC_ORBHESS_TIME set when the library first runs one)
static bool orbhess_timed() { static const bool on = getenv("SQMC_ORBHESS_TIME") != nullptr; return on; }

// what the kernels need beside the context's integrals: pair[a norb + r] = combine_2(a + 1, r + 1), behind it the npair pair indices
// in the kernels' own numbering, and the offset of the one-body block
static int orbhess_tables(const sqmc_gpu_ctx *c, std::vector<int> &tab) {
  const ChemTab &t = c->htab;
  const int n = t.norb, n1 = n + 1, nn = n * n;
  const long long A = t.c2[n1 * t.c2_stride + n1];
  tab.assign((size_t)nn + (size_t)n * n1 / 2, 0);
  for (int p = 0; p < n; p++) for (int q = 0; q < n; q++) tab[(size_t)p * n + q] = t.c2[(p + 1) * t.c2_stride + (q + 1)];
  for (int p = 0; p < n; p++) for (int q = 0; q <= p; q++) tab[(size_t)nn + (size_t)p * (p + 1) / 2 + q] = tab[(size_t)p * n + q];
  return (int)(A * (A - 1) / 2);
}

static int oneidx_door(sqmc_gpu_ctx *c, const double *kappa, double *integrals_out) {
  const char *who = "sqmc_gpu_one_index_transform";
  if (!c || !kappa || !integrals_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_one_index_transform: null argument");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_one_index_transform: chem contexts only (heg, hubbard2 and hubbardk hold no integral table)");
  const int n = c->htab.norb, nn = n * n;
  for (int e = 0; e < nn; e++) if (!std::isfinite(kappa[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_one_index_transform: kappa holds a non-finite entry");
  int rc = rot_check_combine2(c, who);
  if (rc != SQMC_OK) return rc;
  std::vector<int> tab;
  const int hbase = orbhess_tables(c, tab);
  const OrbHessPlan hp = orbhess_plan(n);
  const size_t n_out = (size_t)c->n_ints + 1;
  std::vector<double> host(n_out);       // declared ahead of s: s waits for the stream before the copy's target goes
  hipStream_t st = c->st;
  DevScratch s(st);
  double *d_kap = s.take<double>(nn); int *d_tab = s.take<int>(tab.size());
  double *d_work = s.take<double>((size_t)hp.npair * hp.npair), *d_out = s.take<double>(n_out);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpyAsync(d_kap, kappa, (size_t)nn * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemsetAsync(d_out, 0, n_out * 8, st));      // the core energy and every slot no pair addresses are 0.0
  orbopt_launch_oneidx_half(st, hp, c->d_ints, d_tab, d_tab + nn, hbase, d_kap, n, d_work);
  HIPDOOR(who, hipGetLastError());
  orbopt_launch_oneidx_sym(st, hp, c->d_ints, d_tab, d_tab + nn, hbase, d_kap, n, d_work, d_out);
  HIPDOOR(who, hipGetLastError());
  HIPDOOR(who, hipMemcpyAsync(host.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipStreamSynchronize(st));
  memcpy(integrals_out, host.data(), n_out * 8);      // only a finished table reaches the caller
  return SQMC_OK;
}
int sqmc_gpu_one_index_transform(sqmc_gpu_ctx *c, const double *kappa, double *integrals_out) {
  try { return oneidx_door(c, kappa, integrals_out); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_one_index_transform: out of host memory"); }
}

// The plan: D, G, the tables, F, the gradient and the diagonal Hessian at kappa = 0, and the work space of a product, all resident.
struct sqmc_orbopt_plan {
  sqmc_gpu_ctx *c; int n, hbase; size_t n_out; OrbPlan fp; OrbHessPlan hp;
  double *d_D, *d_G; int *d_tab; double *d_part, *d_F, *d_grad, *d_hd, *d_work, *d_tilde, *d_Ft;
  std::vector<double> F, grad, hd;       // what prepare computed, as sqmc_gpu_orbopt_gradient hands it out
  double ms[4];                          // HIP-event times of the last product: half pass, symmetrising pass with the one-body block, Fock GEMM, sigma
  DevScratch mem;
};
int sqmc_gpu_orbopt_free(sqmc_orbopt_plan *p) {
  if (!p) return SQMC_OK;
  p->mem.clear();                        // waits for the context's stream: the plan goes before its context
  delete p;
  return SQMC_OK;
}
static int orbopt_prepare_door(sqmc_gpu_ctx *c, const double *one_rdm, const double *two_rdm_sf, sqmc_orbopt_plan **plan_out) {
  const char *who = "sqmc_gpu_orbopt_prepare";
  if (!c || !one_rdm || !two_rdm_sf || !plan_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_prepare: null argument");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_orbopt_prepare: chem contexts only (heg, hubbard2 and hubbardk hold no integral table)");
  const int n = c->htab.norb, nn = n * n;
  const size_t n4 = (size_t)nn * nn;
  for (int e = 0; e < nn; e++) if (!std::isfinite(one_rdm[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_prepare: one_rdm holds a non-finite entry");
  for (size_t e = 0; e < n4; e++) if (!std::isfinite(two_rdm_sf[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_prepare: two_rdm_sf holds a non-finite entry");
  int rc = rot_check_combine2(c, who);
  if (rc != SQMC_OK) return rc;
  std::unique_ptr<sqmc_orbopt_plan> p(new sqmc_orbopt_plan());      // value-initialised
  std::vector<int> tab;
  p->c = c; p->n = n; p->hbase = orbhess_tables(c, tab); p->n_out = (size_t)c->n_ints + 1; p->fp = orbopt_plan(n); p->hp = orbhess_plan(n);
  p->F.resize(nn); p->grad.resize(nn); p->hd.resize(nn);
  hipStream_t st = c->st;
  p->mem.stream = st;
  DevScratch s(st);                      // behind p: on an early return it waits for the stream and frees before the plan's host arrays go
  p->d_D = s.take<double>(nn); p->d_G = s.take<double>(n4); p->d_tab = s.take<int>(tab.size());
  p->d_part = s.take<double>((size_t)p->fp.nblocks * nn); p->d_F = s.take<double>(nn); p->d_grad = s.take<double>(nn); p->d_hd = s.take<double>(nn);
  p->d_work = s.take<double>((size_t)p->hp.npair * p->hp.npair); p->d_tilde = s.take<double>(p->n_out); p->d_Ft = s.take<double>(nn);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpyAsync(p->d_D, one_rdm, (size_t)nn * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemcpyAsync(p->d_G, two_rdm_sf, n4 * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemcpyAsync(p->d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  // the launches of sqmc_gpu_orbital_gradient with all three outputs, in its order: the same bits
  orbopt_launch_fock(st, p->fp, c->d_ints, p->d_tab, p->hbase, p->d_D, p->d_G, n, p->d_part, p->d_F);
  HIPDOOR(who, hipGetLastError());
  orbopt_launch_grad(st, p->d_F, n, p->d_grad);
  HIPDOOR(who, hipGetLastError());
  orbopt_launch_hdiag(st, c->d_ints, p->d_tab, p->hbase, p->d_D, p->d_G, p->d_F, n, p->d_hd);
  HIPDOOR(who, hipGetLastError());
  HIPDOOR(who, hipMemcpyAsync(p->F.data(), p->d_F, (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipMemcpyAsync(p->grad.data(), p->d_grad, (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipMemcpyAsync(p->hd.data(), p->d_hd, (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipStreamSynchronize(st));
  for (void *q : {(void *)p->d_D, (void *)p->d_G, (void *)p->d_tab, (void *)p->d_part, (void *)p->d_F, (void *)p->d_grad, (void *)p->d_hd, (void *)p->d_work,
                  (void *)p->d_tilde, (void *)p->d_Ft}) s.keep(q, p->mem);
  *plan_out = p.release();
  return SQMC_OK;
}
int sqmc_gpu_orbopt_prepare(sqmc_gpu_ctx *c, const double *one_rdm, const double *two_rdm_sf, sqmc_orbopt_plan **plan_out) {
  try { return orbopt_prepare_door(c, one_rdm, two_rdm_sf, plan_out); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_orbopt_prepare: out of host memory"); }
}
int sqmc_gpu_orbopt_gradient(sqmc_orbopt_plan *p, double *fock_out, double *grad_out, double *hdiag_out) {
  if (!p) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_gradient: null plan");
  if (!fock_out && !grad_out && !hdiag_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_gradient: all three outputs are null");
  const size_t bytes = (size_t)p->n * p->n * 8;
  if (fock_out) memcpy(fock_out, p->F.data(), bytes);
  if (grad_out) memcpy(grad_out, p->grad.data(), bytes);
  if (hdiag_out) memcpy(hdiag_out, p->hd.data(), bytes);
  return SQMC_OK;
}
static int orbopt_hv_door(sqmc_orbopt_plan *p, const double *kappa, double *sigma_out) {
  const char *who = "sqmc_gpu_orbopt_hessian_vector";
  if (!p || !kappa || !sigma_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_hessian_vector: null argument");
  sqmc_gpu_ctx *c = p->c;
  const int n = p->n, nn = n * n;
  for (int e = 0; e < nn; e++) if (!std::isfinite(kappa[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_hessian_vector: kappa holds a non-finite entry");
  for (int a = 0; a < n; a++)
    for (int b = 0; b <= a; b++)
      if (kappa[a * n + b] != -kappa[b * n + a]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_orbopt_hessian_vector: kappa is not antisymmetric (kappa[p,q] == -kappa[q,p], zero diagonal)");
  std::vector<double> host((size_t)nn);  // declared ahead of s
  hipStream_t st = c->st;
  DevScratch s(st);
  double *d_kap = s.take<double>(nn), *d_sig = s.take<double>(nn);
  if (!s.ok()) return hip_fail(who, s.err());
  const int *d_pair = p->d_tab, *d_pidx = p->d_tab + nn;
  HIPDOOR(who, hipMemcpyAsync(d_kap, kappa, (size_t)nn * 8, hipMemcpyHostToDevice, st));
  HIPDOOR(who, hipMemsetAsync(p->d_tilde, 0, p->n_out * 8, st));
  EventMarks ev1(orbhess_timed(), 3), ev2(orbhess_timed(), 3);      // four stages: two owners of up to four events each, sharing the middle point
  HIPDOOR(who, ev1.mark(st));
  orbopt_launch_oneidx_half(st, p->hp, c->d_ints, d_pair, d_pidx, p->hbase, d_kap, n, p->d_work);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev1.mark(st));
  orbopt_launch_oneidx_sym(st, p->hp, c->d_ints, d_pair, d_pidx, p->hbase, d_kap, n, p->d_work, p->d_tilde);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev1.mark(st)); HIPDOOR(who, ev2.mark(st));
  orbopt_launch_fock(st, p->fp, p->d_tilde, d_pair, p->hbase, p->d_D, p->d_G, n, p->d_part, p->d_Ft);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev2.mark(st));
  orbopt_launch_sigma(st, p->d_Ft, p->d_grad, d_kap, n, d_sig);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev2.mark(st));
  HIPDOOR(who, hipMemcpyAsync(host.data(), d_sig, (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPDOOR(who, hipStreamSynchronize(st));
  p->ms[0] = p->ms[1] = p->ms[2] = p->ms[3] = 0.0;
  ev1.add(p->ms); ev2.add(p->ms + 2);
  memcpy(sigma_out, host.data(), (size_t)nn * 8);      // only a finished product reaches the caller
  return SQMC_OK;
}
int sqmc_gpu_orbopt_hessian_vector(sqmc_orbopt_plan *p, const double *kappa, double *sigma_out) {
  try { return orbopt_hv_door(p, kappa, sigma_out); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_orbopt_hessian_vector: out of host memory"); }
}
// milliseconds the stages of the plan's last product took: the half pass, the symmetrising pass with the one-body block, the Fock GEMM
// on the transformed table with its reduction, the sigma kernel (0 unless SQMC_ORBHESS_TIME was set when the library first ran a
// product); not part of the ABI
int sqmc_gpu_debug_orbhess_ms(sqmc_orbopt_plan *p, double out[4]) {
  if (!p || !out) return SQMC_ERR_BAD_ARG;
  for (int k = 0; k < 4; k++) out[k] = p->ms[k];
  return SQMC_OK;
}
// the shape of the one-index transformation at norb orbitals: register tile of the half pass, side of the symmetrising tile, pairs,
// blocks of the symmetrising pass; not part of the ABI
int sqmc_gpu_debug_orbhess_plan(int32_t norb, int64_t out[4]) {
  if (norb < 1 || norb > SQ_MAXORB || !out) return SQMC_ERR_BAD_ARG;
  const OrbHessPlan p = orbhess_plan(norb);
  out[0] = p.tm; out[1] = ORB_SYM_TILE; out[2] = p.npair; out[3] = p.nsym;
  return SQMC_OK;
}
