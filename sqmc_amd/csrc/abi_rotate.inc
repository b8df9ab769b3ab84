// abi_rotate.inc -- C-ABI entry point of the integral rotation (inside extern "C"); kernels in rotate_kernels.h
// Textually included by sqmc_gpu.hip; not a standalone file.

// tools/rotate_time.py: HIP events around the three kernels (SQMC_ROT_TIME set when the library first runs a rotation)
static bool rot_timed() { static const bool on = getenv("SQMC_ROT_TIME") != nullptr; return on; }

extern "C++" {
template <int MODE, int TM>
static hipError_t rot_launch(sqmc_gpu_ctx *c, int blocks, size_t lds, const double *rot, const double *src, double *dst) {
  void (*k)(ChemDev, const double *, const double *, double *, int) = k_rot<MODE, TM>;
  if (lds > 64 * 1024) { hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(k, dim3(blocks), dim3(ROT_T), lds, c->st, c->dev, rot, src, dst, c->htab.norb);
  return hipGetLastError();
}
template <int MODE>
static hipError_t rot_launch_mode(sqmc_gpu_ctx *c, int blocks, size_t lds, const double *rot, const double *src, double *dst) {
  // 4 x 4 register tiles fill the 256 threads from 33 orbitals on; below that 2 x 2 tiles keep more of them busy
  return c->htab.norb > 32 ? rot_launch<MODE, 4>(c, blocks, lds, rot, src, dst) : rot_launch<MODE, 2>(c, blocks, lds, rot, src, dst);
}
}

// the kernels address the table through combine_2: every index they form must lie inside it, and no two pairs may share a slot
// (also the test of sqmc_gpu_orbital_gradient, abi_orbopt.inc)
static int rot_check_combine2(const sqmc_gpu_ctx *c, const char *who) {
  const ChemTab &t = c->htab;
  const int n = t.norb, n1 = n + 1;
  const long long A = t.c2[n1 * t.c2_stride + n1];
  std::vector<char> seen((size_t)A + 1, 0);
  for (int p = 1; p <= n; p++)
    for (int q = 1; q <= p; q++) {
      const int a = t.c2[p * t.c2_stride + q];
      if (a < 1 || a >= A || a != t.c2[q * t.c2_stride + p] || seen[a]) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": combine_2 is not a symmetric one-to-one pair index below combine_2(norb+1, norb+1)");
      seen[a] = 1;
    }
  if (A * (A - 1) / 2 + A > c->n_ints) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": integral table shorter than integral_index(norb+1,...)");
  return SQMC_OK;
}

int sqmc_gpu_rotate_integrals(sqmc_gpu_ctx *c, const double *rot, double *integrals_out) {
  if (!c || !rot || !integrals_out) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_rotate_integrals: null argument");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "sqmc_gpu_rotate_integrals: chem contexts only (heg, hubbard2 and hubbardk hold no integral table)");
  const ChemTab &t = c->htab;
  const int n = t.norb, n1 = n + 1, nn = n * n;
  for (int e = 0; e < nn; e++) if (!std::isfinite(rot[e])) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_rotate_integrals: rot holds a non-finite entry");
  const long long npair = (long long)n * n1 / 2;
  int rc = rot_check_combine2(c, "sqmc_gpu_rotate_integrals");
  if (rc != SQMC_OK) return rc;
  const size_t n_out = (size_t)c->n_ints + 1, lds = (size_t)3 * nn * sizeof(double);
  const char *who = "sqmc_gpu_rotate_integrals";
  std::vector<double> host(n_out);
  c->rot_ms[0] = c->rot_ms[1] = c->rot_ms[2] = 0.0;
  DevScratch s(c->st);
  double *d_rot = s.take<double>(nn), *d_work = s.take<double>((size_t)npair * npair), *d_out = s.take<double>(n_out);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpy(d_rot, rot, (size_t)nn * 8, hipMemcpyHostToDevice));
  HIPDOOR(who, hipMemsetAsync(d_out, 0, n_out * 8, c->st));      // every slot no kernel addresses is 0.0
  EventMarks ev(rot_timed(), 4);
  HIPDOOR(who, ev.mark(c->st));
  HIPDOOR(who, rot_launch_mode<ROT_HALF1>(c, (int)npair, lds, d_rot, c->d_ints, d_work));
  HIPDOOR(who, ev.mark(c->st));
  HIPDOOR(who, rot_launch_mode<ROT_HALF2>(c, (int)npair, lds, d_rot, d_work, d_out));
  HIPDOOR(who, ev.mark(c->st));
  HIPDOOR(who, rot_launch_mode<ROT_ONE>(c, 1, lds, d_rot, c->d_ints, d_out));
  HIPDOOR(who, ev.mark(c->st));
  HIPDOOR(who, hipMemcpyAsync(host.data(), d_out, n_out * 8, hipMemcpyDeviceToHost, c->st));
  HIPDOOR(who, hipStreamSynchronize(c->st));
  ev.add(c->rot_ms);
  memcpy(integrals_out, host.data(), n_out * 8);      // only a finished table reaches the caller
  return SQMC_OK;
}
// milliseconds the kernels of the last rotation took: half 1, half 2, the one-body block (0 unless SQMC_ROT_TIME was set when the library
// first ran one); not part of the ABI
int sqmc_gpu_debug_rotate_ms(sqmc_gpu_ctx *c, double *half1_ms, double *half2_ms, double *one_body_ms) {
  if (!c || !half1_ms || !half2_ms || !one_body_ms) return SQMC_ERR_BAD_ARG;
  *half1_ms = c->rot_ms[0]; *half2_ms = c->rot_ms[1]; *one_body_ms = c->rot_ms[2];
  return SQMC_OK;
}
