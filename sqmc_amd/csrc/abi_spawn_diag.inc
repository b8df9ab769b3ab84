// Spawn diagnostics: the walk's histograms of abs(weight_j)/tau and its max / min weight ratios (do_walk.f90:104, 1420-1429, 3619-3661,
// add_walker 7603-7636; printed at 3295-3320).  k_spawn's diagnostic form fills them (walk_kernels.h: sdiag_record).
//
// The totals after N returned steps hold exactly the proposals of those N steps: while the diagnostics are on no head is enqueued
// ahead of its step (sqmc_gpu_step and run_steps clear pipeline_next), so every k_spawn launch belongs to a step that is then
// finished; a bucket tail that gives up is re-run through the radix tail on the spawns that are already there, without a second
// k_spawn launch.  Trajectories do not depend on the pipelining.
// d_sdiag: SDIAG_REPL sets the spawning blocks add to, and behind them the set k_sdiag_reduce folds them into
static int sdiag_clear(sqmc_gpu_ctx *c) { HIPCHK(hipMemset(c->d_sdiag, 0, (size_t)(SDIAG_REPL + 1) * SDIAG_WORDS * 8)); return SQMC_OK; }
int sqmc_gpu_set_spawn_diagnostics(sqmc_gpu_ctx *c, int32_t on) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (c->sdiag_on == (on != 0)) return SQMC_OK;      // nothing changes (a host that repeats the call per block): a pending head stays valid
  abandon_head(c);      // a head enqueued for the next step was launched in the other form
  HIPCHK(hipStreamSynchronize(c->st));
  if (on && !c->d_sdiag) {
    HIPCHK(hipMalloc(&c->d_sdiag, (size_t)(SDIAG_REPL + 1) * SDIAG_WORDS * 8));
    if (int r = sdiag_clear(c)) { hipFree(c->d_sdiag); c->d_sdiag = nullptr; return r; }
  }
  c->sdiag_on = on != 0;
  return SQMC_OK;
}
int sqmc_gpu_reset_spawn_diagnostics(sqmc_gpu_ctx *c) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (!c->d_sdiag) return SQMC_OK;
  HIPCHK(hipStreamSynchronize(c->st)); HIPCHK(hipStreamSynchronize(c->st2)); HIPCHK(hipStreamSynchronize(c->st3));
  return sdiag_clear(c);
}
int sqmc_gpu_get_spawn_diagnostics(sqmc_gpu_ctx *c, int32_t *nbins, int64_t *bins, int64_t *bins_hf, int64_t *bins_single, int64_t *bins_double,
                                   double max_ratio_by_level[8], double *max_ratio, int32_t *max_ratio_level, double *min_ratio, int64_t *n_nan) {
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (!c->d_sdiag) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_get_spawn_diagnostics: sqmc_gpu_set_spawn_diagnostics was never switched on");
  HIPCHK(hipStreamSynchronize(c->st)); HIPCHK(hipStreamSynchronize(c->st2)); HIPCHK(hipStreamSynchronize(c->st3));
  u64 *tot = c->d_sdiag + (size_t)SDIAG_REPL * SDIAG_WORDS;
  hipLaunchKernelGGL(k_sdiag_reduce, dim3(nblk(SDIAG_WORDS)), dim3(TPB), 0, c->st, (const u64 *)c->d_sdiag, tot);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
  if (nbins) *nbins = SDIAG_NB;
  int64_t *outs[4] = {bins, bins_hf, bins_single, bins_double};
  for (int k = 0; k < 4; k++) if (outs[k]) HIPCHK(hipMemcpy(outs[k], tot + (long long)k * SDIAG_NB, SDIAG_NB * 8, hipMemcpyDeviceToHost));
  u64 tail[10];
  HIPCHK(hipMemcpy(tail, tot + SDIAG_MAX, sizeof(tail), hipMemcpyDeviceToHost));
  // max_wt_ratio = -1.d99, min_wt_ratio = 1.d99 until a proposal qualifies (do_walk.f90:3432-3433)
  double best = -1e99; int lev = -1;
  for (int l = 0; l < 8; l++) {
    double v = -1e99; if (tail[l]) memcpy(&v, &tail[l], 8);
    if (max_ratio_by_level) max_ratio_by_level[l] = v;
    if (v > best) { best = v; lev = l; }      // the lowest level that attains the maximum
  }
  if (max_ratio) *max_ratio = best;
  if (max_ratio_level) *max_ratio_level = lev;
  if (min_ratio) { double v = 1e99; if (tail[8]) { const u64 b = ~tail[8]; memcpy(&v, &b, 8); } *min_ratio = v; }      // kept as the complement: walk_kernels.h
  if (n_nan) *n_nan = (int64_t)tail[9];
  return SQMC_OK;
}
