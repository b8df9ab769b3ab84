// abi_shard.inc -- C-ABI entry points of the multi-rank sharded step and the in-library RCCL exchange (inside extern "C")
// Textually included by sqmc_gpu.hip (one translation unit: the kernels share the ChemTab LDS
// image, the walker SoA types and the launch helpers defined there); not a standalone header.

// ------------------------------------------------------------------ multi-rank sharding
static int psit_shard_exchange(sqmc_gpu_ctx *c);                                                          // hf_to_psit over ranks (end of file)
static int psit_shard_project(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const double *x_global_dev);
// owner of a determinant (the role of get_det_owner, mpi_routines.f90:419-445; any hash will
// do for ownership, SURVEY.md section 5)
__global__ void __launch_bounds__(TPB) k_owner_batch(ChemDev dev, const u64 *up, const u64 *dn, int *owner, long long n, int nranks, int mode) {
  long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i < n) owner[i] = det_owner_any(mode, mode == SQMC_OWNER_DJB ? 0ull : det_key(dev, up[i], dn[i]), up[i], dn[i], nranks);
}
// x_global(grow(k)) = w(loc(k)) for the deterministic-space walkers this rank owns
__global__ void __launch_bounds__(TPB) k_prj_gather_rows(const double *__restrict__ wt, const int *__restrict__ loc, const int *__restrict__ grow,
                                                         double *__restrict__ xg, long long n) {
  long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i < n) xg[grow[i]] = wt[loc[i]];
}
// the whole vector in one pass -- this rank's rows, zeros for the others' (no memset in front) -- and, with `tail`, this rank's share of
// the step's sums behind it (one all-reduce carries both)
__global__ void __launch_bounds__(TPB) k_prj_gather_all(const double *__restrict__ wt, const int *__restrict__ loc, const int *__restrict__ ginv,
                                                        double *__restrict__ xg, long long n_imp, const double *redl, double *__restrict__ tail,
                                                        FinArgs fin, DevScalars *sc) {
  // redl is DevScalars::redl, which finish_all (block 0) WRITES just above the copy below: no __restrict__ on it -- the load must stay
  // behind finish_all's closing barrier
  if (fin.on && blockIdx.x == 0) finish_all(fin, sc);        // the step's final sums (k_finish's work: same block shape, same order), then their copy below
  long long g = (long long)blockIdx.x * TPB + threadIdx.x;
  if (g < n_imp) { const int i = ginv[g]; xg[g] = i >= 0 ? wt[loc[i]] : 0.0; }
  if (tail && g < 8) tail[g] = ((const volatile double *)redl)[g];
}
// rows owned by this rank of y = A x_global, same ordered accumulation as k_prj_apply
__global__ void __launch_bounds__(TPB) k_prj_apply_rows(const int *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                        const double *__restrict__ xg, const int *__restrict__ loc, const int *__restrict__ grow,
                                                        double *__restrict__ wt, long long n, double e_trial, double tau) {
  __shared__ double sprod[TPB / 64][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * (TPB / 64) + wv;
  if (i >= n) return;
  const int row = grow[i];
  const int b = ptr[row], e = ptr[row + 1];
  double y = 0.0;
  for (int base = b; base < e; base += 64) {
    const int k = base + lane;
    sprod[wv][lane] = (k < e) ? val[k] * xg[col[k]] : 0.0;
    __builtin_amdgcn_wave_barrier();
    const int cnt = (e - base < 64) ? (e - base) : 64;
    for (int l = 0; l < cnt; l++) y = y + sprod[wv][l];
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) { y = y + e_trial * tau * xg[row]; wt[loc[i]] = wt[loc[i]] + y; }
}
// the last line of the projection for the rows this rank owns, y = A x_global already there (spare blocks of the head's k_spawn):
// k_prj_apply_rows's closing statements
__global__ void __launch_bounds__(TPB) k_prj_finish_rows(const double *__restrict__ yv, const double *__restrict__ xg, const int *__restrict__ loc, const int *__restrict__ grow,
                                                         double *__restrict__ wt, long long n, double e_trial, double tau) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int row = grow[i];
  double y = yv[i];
  y = y + e_trial * tau * xg[row]; wt[loc[i]] = wt[loc[i]] + y;
}
// destination rank of every spawn slot (nranks = "no walker": weight 0), as an 8-bit sort key; a slot is a child, or with
// fast_heatbath one of a child's two walker slots (each routed by its own determinant: the two may go to different ranks)
// (koff: hf_to_psit's offset of the sort keys outside C(T), taken off again -- the owner is the determinant's)
__global__ void __launch_bounds__(TPB) k_child_owner(WalkArr w, const u64 *__restrict__ keys, u64 *__restrict__ okey, u32 *__restrict__ oval,
                                                     long long n0, long long nslot, u64 invalid_key, int nranks, int pack, int mode, u64 koff) {
  long long c = (long long)blockIdx.x * TPB + threadIdx.x;
  if (c >= nslot) return;
  u64 k = get_key(keys, n0 + c, pack);
  if (koff && k != invalid_key && k >= koff) k -= koff;
  u64 o = (u64)nranks;
  if (k != invalid_key) { if (mode == SQMC_OWNER_DJB) { const SpawnRec r = w.sp[c]; o = (u64)det_owner_djb(r.up, r.dn, nranks); } else o = (u64)det_owner(k, nranks); }
  okey[c] = o; oval[c] = (u32)c;
}
// 32-byte wire record {up, dn, weight bits, flags}: the t_walk of mpi_routines.f90:29-34 without
// the fields that are sentinels for fresh spawns
// (counts != null: the first block also writes this rank's row of the count all-gather -- k_fill_counts's work, one launch less)
__global__ void __launch_bounds__(TPB) k_pack_send(WalkArr w, const u32 *__restrict__ order, u64 *__restrict__ rec, long long n0, long long nsend,
                                                   const u32 *__restrict__ rowtot = nullptr, int P = 0, u32 room = 0, u32 *__restrict__ counts = nullptr) {
  if (counts && blockIdx.x == 0) {
    for (int k = threadIdx.x; k < P; k += TPB) counts[k] = rowtot[k];
    if (threadIdx.x == 0) { counts[P] = 0u; counts[P + 1] = room; }
  }
  long long q = (long long)blockIdx.x * TPB + threadIdx.x;
  if (q >= nsend) return;
  const long long k = n0 + order[q];
  const SpawnRec r = w.sp[k - n0];
  rec[4 * q] = r.up; rec[4 * q + 1] = r.dn; rec[4 * q + 2] = (u64)__double_as_longlong(r.wt); rec[4 * q + 3] = r.flg;
}
__global__ void __launch_bounds__(TPB) k_unpack_recv(ChemDev dev, WalkArr w, const u64 *__restrict__ rec, u64 *__restrict__ keys, u32 *__restrict__ vals,
                                                     long long n0, long long nrecv, int pack, const u64 *__restrict__ self_rec, long long self_lo, long long self_hi) {
  long long q = (long long)blockIdx.x * TPB + threadIdx.x;
  if (q >= nrecv) return;
  const long long k = n0 + q;
  // records [self_lo, self_hi) are this rank's own bucket: they are read where k_pack_send left them (no copy into the receive buffer)
  const u64 *src = (self_rec && q >= self_lo && q < self_hi) ? self_rec + 4 * (q - self_lo) : rec + 4 * q;
  const u64 u = src[0], d = src[1];
  SpawnRec r; r.up = u; r.dn = d; r.wt = __longlong_as_double((long long)src[2]); r.flg = src[3] & 0xFFFFFFFFull;
  w.sp[q] = r;
  u64 key = det_key(dev, u, d);
  if (dev.ps.koff) key = psit_key(dev.ps, key);      // hf_to_psit: a determinant of this rank's C(T) share sorts into its segment
  put_key(keys, vals, k, key, pack);
}

int sqmc_gpu_det_owner(sqmc_gpu_ctx *c, int64_t n, const uint64_t *up, const uint64_t *dn, int32_t nranks, int32_t *owner) {
  if (!c || nranks < 1 || nranks > 255) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (n <= 0) return SQMC_OK;
  u64 *du, *dd; int *dout;
  HIPCHK(hipMalloc(&du, n * 8)); HIPCHK(hipMalloc(&dd, n * 8)); HIPCHK(hipMalloc(&dout, n * 4));
  HIPCHK(hipMemcpy(du, up, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dd, dn, n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_owner_batch, dim3(nblk(n)), dim3(TPB), 0, c->st, c->dev, du, dd, dout, (long long)n, (int)nranks, c->owner_mode);
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipMemcpy(owner, dout, n * 4, hipMemcpyDeviceToHost));
  hipFree(du); hipFree(dd); hipFree(dout);
  return SQMC_OK;
}

int sqmc_gpu_set_owner_hash(sqmc_gpu_ctx *c, int32_t mode) {
  if (!c || (mode != SQMC_OWNER_MIX && mode != SQMC_OWNER_DJB)) return fail(SQMC_ERR_BAD_ARG, "owner hash: 0 (mix of the sort key) or 1 (the reference's djb_hash)");
  c->owner_mode = mode;
  return SQMC_OK;
}

// hf_to_psit over ranks: the 2P slots of row partials behind x_global (0 for every other walk)
static long long psit_x_extra(const sqmc_gpu_ctx *c) { return c->psit_shard ? 2ll * c->shard_n : 0ll; }

int sqmc_gpu_shard_config(sqmc_gpu_ctx *c, int32_t rank, int32_t nranks, int64_t n_imp_local, const int32_t *global_row) {
  if (!c || nranks < 1 || nranks > 255 || rank < 0 || rank >= nranks || n_imp_local < 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (c->psit_on) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit is built for one rank only");
  if (n_imp_local > 0 && (!global_row || !c->d_prj_ptr)) return fail(SQMC_ERR_BAD_ARG, "set the (global) projector before shard_config");
  for (long long i = 0; i < n_imp_local; i++) if (global_row[i] < 0 || global_row[i] >= c->n_imp) return fail(SQMC_ERR_BAD_ARG, "global row out of range");
  c->shard_rank = rank; c->shard_n = nranks; c->n_imp_local = n_imp_local;
  hipFree(c->d_grow); hipFree(c->d_loc_imp);
  HIPCHK(hipMalloc(&c->d_grow, (n_imp_local + 1) * 4)); HIPCHK(hipMalloc(&c->d_loc_imp, (std::max<long long>(n_imp_local, c->n_imp) + 1) * 4));
  if (n_imp_local > 0) HIPCHK(hipMemcpy(c->d_grow, global_row, n_imp_local * 4, hipMemcpyHostToDevice));
  // the inverse map: which of this rank's deterministic walkers is global row g (-1: another rank's)
  hipFree(c->d_ginv); c->d_ginv = nullptr;
  if (c->n_imp > 0) {
    std::vector<int> inv((size_t)c->n_imp, -1);
    for (long long i = 0; i < n_imp_local; i++) {
      if (inv[global_row[i]] >= 0) return fail(SQMC_ERR_BAD_ARG, "global row named twice");
      inv[global_row[i]] = (int)i;
    }
    HIPCHK(hipMalloc(&c->d_ginv, c->n_imp * 4)); HIPCHK(hipMemcpy(c->d_ginv, inv.data(), c->n_imp * 4, hipMemcpyHostToDevice));
  }
  return SQMC_OK;
}

// phase 1 of a sharded step: gate, child offsets, death/clone, spawn (into local slots), and the
// owned entries of the deterministic-space weight vector written into x_global (device pointer,
// n_imp doubles, zeroed here) for the caller's all-reduce (do_walk.f90:2259-2260).
static int shard_begin_impl(sqmc_gpu_ctx *c, const sqmc_step_params *sp, double *x_global_dev, int64_t *n_children, bool full_sync, bool side = false, bool diag_side = false) {
  if (!c || !sp || !n_children) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (c->shard_n < 1 || !c->d_grow) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_shard_config not called");
  if (c->rng_mode != SQMC_RNG_COUNTER) return fail(SQMC_ERR_UNSUPPORTED, "sharded steps need the COUNTER RNG discipline");
  if (!c->d_ct_up) return fail(SQMC_ERR_UNSUPPORTED, "sharded step: the C(T) table must be set");
  // semistochastic = f (do_walk.f90:2475: join_walker2 is local to a rank): the same three phases without the projection
  if (!sp->semistochastic && (c->n_imp > 0 || c->n_imp_local > 0)) return fail(SQMC_ERR_BAD_ARG, "sharded plain walk: no projector may be set (sqmc_gpu_shard_config with no rows)");
  if (c->mwalk <= 0) return fail(SQMC_ERR_BAD_ARG, "no walker arrays");
  hipStream_t st = c->st;
  const StepP p = step_params(c, sp);
  if (c->psit_on) {
    if (!sp->semistochastic) return fail(SQMC_ERR_BAD_ARG, "hf_to_psit needs a semistochastic step");
    if (c->nwalk < p.nct) return fail(SQMC_ERR_BAD_ARG, "hf_to_psit: the walker list does not hold this rank's C(T) share");
  }
  const long long n0 = c->nwalk, M = c->mwalk;
  const long long nx = c->n_imp + psit_x_extra(c);        // hf_to_psit: 2P slots of row partials behind the weights
  ScanWork sw0; sw0.state = c->d_scan_state; sw0.ticket = c->d_scan_ticket; sw0.cap_tiles = c->cap_tiles; sw0.self_clear = false;
  collect_timers(c);
  c->nt = 0;
  if (n0 == 0) HIPCHK(hipMemsetAsync(&c->d_sc->n_children, 0, 4 * sizeof(u64) + 2 * sizeof(int), st));   // otherwise k_gate clears them
  // side = the in-library step with a second communicator: death/clone, the gather of the owned
  // deterministic weights (and later their all-reduce and the projection) run on the side stream
  // beside k_spawn, the bucketing of the spawns and their exchange
  hipStream_t sx = side ? c->st2 : st;
  // x_ready: every rank all-reduced the deterministic weights for this step behind the last step's sums (a collective all of them
  // issue or none does); y_ok: this rank's pipelined head also multiplied its projector rows into them
  const bool x_ready = c->shard_x_ready && x_global_dev == c->d_xg;
  const bool y_ok = x_ready && c->head_ready && c->shard_y_ok;
  c->shard_x_ready = false;
  if (!side && !x_ready && x_global_dev && c->n_imp > 0) HIPCHK(hipMemsetAsync(x_global_dev, 0, nx * 8, st));
  const bool mail = (n0 > 0 && M > n0);
  u64 cseq;
  if (c->head_ready) {
    // gate + scan + spawn of this step already run behind the last step's mail (pipelined head of sqmc_gpu_shard_run);
    // with one stream they simply sit in front of this step's death/clone and projection in stream order
    int rt = take_head(c, n0 > 0 && M > n0 && head_fits(c->head_p, p), "internal: the pipelined head of this sharded step does not fit it", -1, -1, &cseq); if (rt) return rt;
    if (spawn_events_on(c, c->step_no, p.semi) && c->nt < NTIMERS) { const int t = c->nt++; c->tname[t] = "spawn"; std::swap(c->ev0[t], c->hev[2]); std::swap(c->ev1[t], c->hev[3]); }
  } else {
    cseq = ++c->cnt_seq;
    if (n0 > 0) {
      hipLaunchKernelGGL(k_gate, dim3(nblk(n0)), dim3(TPB), 0, st, c->dev, c->w.up, c->w.dn, c->w.wt, c->d_nchild, c->d_wchild, c->d_keys, c->d_vals,
                         n0, p, c->seed64, c->step_no, c->d_sc, c->pack, 0, FinArgs{});
      c->scan_used[0] = device_excl_scan_u64(c->d_nchild, c->d_child_off, n0, &c->d_sc->n_children, sw0, st);
      c->scan_flip = 1;        // as enqueue_head: look-back set 0 is in use until the step's finish
    }
    if (side || diag_side) { HIPCHK(hipEventRecord(c->e_fork, st)); c->fork_valid = true; }
    if (n0 > 0) {
      TBEG(spawn, st);
      if (M > n0)      // first: it posts the child count to the host mailbox as soon as it starts
        launch_spawn(c, spawn_kind(c), 0, (unsigned)nblk(M - n0), 0, nullptr, nullptr, p, c->step_no, n0, cseq, 0, shard_owner_out(c), BucketArgs{}, FinArgs{}, PrjPre{}, 0);
      TEND(spawn, st);
    }
  }
  if (side) {
    HIPCHK(hipStreamWaitEvent(sx, c->e_fork, 0));
    if (x_global_dev && c->n_imp > 0) HIPCHK(hipMemsetAsync(x_global_dev, 0, c->n_imp * 8, sx));
  }
  // diag_side (the in-library step with ONE communicator): death/clone alone goes to the side stream -- no collective runs there -- and
  // overlaps the projection, the bucketing of the spawns and their exchange; it touches no deterministic-space weight, they touch no other
  if (diag_side && !side && n0 > 0) {
    if (!c->fork_valid) { HIPCHK(hipEventRecord(c->e_fork, st)); c->fork_valid = true; }      // (a pipelined head recorded it in front of its kernels)
    HIPCHK(hipStreamWaitEvent(c->st2, c->e_fork, 0));
  }
  if (n0 > 0) {
    hipLaunchKernelGGL(k_diag, dim3(nblk(n0)), dim3(TPB), 0, (diag_side && !side) ? c->st2 : sx, c->dev, c->w.up, c->w.dn, c->w.wt, c->w.flg, c->w.me, n0, p, c->d_sc, 0);
    if (diag_side && !side) {
      // the short-list tail's bucket boundaries for this step (bucket_partition.h): where the current set lies in this step's
      // resident list and the next set from the last tail's counts -- a chain of dependent loads that has the whole exchange to hide in
      memset(&c->shard_ba, 0, sizeof(c->shard_ba));
      if (bucket_static_ok(c, p) && c->residents_sorted && c->bk_holdoff == 0 && c->last_nall > 0 && c->last_nall < (1ll << 20) && n0 >= 256) {
        long long B = bucket_count(c->last_nall); if (B > n0) B = n0;
        BucketArgs hb; memset(&hb, 0, sizeof(hb));
        hb.B = (int)B; hb.scount = c->d_bscount;
        c->head_kb_use = choose_boundaries(c, B, n0, hb);
        if (hb.kb || hb.kb_out) hipLaunchKernelGGL(k_bucket_boundaries, dim3(2), dim3(BK_T), 0, c->st2, (const u64 *)c->d_keys, n0, hb);
        c->shard_ba = hb;
      }
      HIPCHK(hipEventRecord(c->e_join, c->st2));
    }
    if (c->n_imp_local > 0 && !x_ready)
      hipLaunchKernelGGL(k_prj_gather_rows, dim3(nblk(c->n_imp_local)), dim3(TPB), 0, sx, c->w.wt, c->d_loc_imp, c->d_grow, x_global_dev, c->n_imp_local);
    if (c->psit_shard && x_global_dev) {       // do_walk.f90:2285-2286 over ranks: this rank's partials of the first row, reduced with the weights
      const PsitArgs &a = c->psit;
      if (!a.seq && a.n_ct > 0) hipLaunchKernelGGL(k_psit_ct_terms, dim3((unsigned)((a.n_ct + 4095) / 4096)), dim3(64), 0, sx, a, (const double *)c->w.wt);
      hipLaunchKernelGGL(k_psit_row_parts, dim3(1), dim3(128), 0, sx, a, (const double *)c->w.wt, x_global_dev + c->n_imp, p.tau, p.e_trial);
    }
  }
  c->shard_y_used = y_ok; c->shard_x_used = x_ready;
  HIPCHK(hipGetLastError());
  long long nch = 0;
  int wr = mail ? wait_mail(&c->h_mail->cnt_seq, cseq, st) : -1;
  if (wr > 0) return mail_fail(wr);
  if (wr == 0) nch = (long long)c->h_mail->n_children;
  else if (n0 > 0) { u64 v; HIPCHK(hipMemcpyAsync(&v, &c->d_sc->n_children, 8, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st)); nch = (long long)v; }
  if (full_sync) HIPCHK(hipStreamSynchronize(st));      // the caller's collective library reads x_global on its own stream
  const long long spc = c->dev.hb.on ? 2 : 1;          // walker slots per child (fast_heatbath: two), as in sqmc_gpu_step
  if (n0 + spc * nch > M) {      // (k_spawn checked the same on the device and wrote nothing, a pipelined head's included)
    reset_scan_words(c);
    return fail(SQMC_ERR_MWALK, "nwalk>MWALK");
  }
  c->shard_n0 = n0; c->shard_nch = nch; c->shard_nslot = spc * nch;
  *n_children = nch;
  return SQMC_OK;
}

int sqmc_gpu_shard_begin(sqmc_gpu_ctx *c, const sqmc_step_params *sp, double *x_global_dev, int64_t *n_children) {
  return shard_begin_impl(c, sp, x_global_dev, n_children, true);
}

// phase 2: apply the owned rows of the deterministic projection with the all-reduced x_global, then
// bucket this step's spawn slots by owner rank (stable) into 32-byte records: send_counts[r] records
// for rank r, contiguous in rank order in send_dev (capacity cap_records).  A step has shard_nslot = spc * nch
// slots: one per child, two with fast_heatbath (the single and the double excitation of a proposal).
//
// device part of phase 2; leaves the per-destination counts in d_rowtot[0..P) (valid when there are slots)
// and the permutation of the slots by destination in *order.  Slots that hold no
// walker sort behind the last rank: they are neither counted nor sent.
static int shard_bucket(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const double *x_global_dev, u32 **order, bool apply_rows = true) {
  hipStream_t st = c->st;
  const long long n0 = c->shard_n0, nsl = c->shard_nslot; const int P = c->shard_n;
  if (apply_rows && c->psit_shard) { int r = psit_shard_project(c, sp, x_global_dev); if (r) return r; }
  else if (apply_rows && c->n_imp_local > 0 && c->shard_y_used)
    hipLaunchKernelGGL(k_prj_finish_rows, dim3(nblk(c->n_imp_local)), dim3(TPB), 0, st, (const double *)c->d_prj_y, x_global_dev, c->d_loc_imp, c->d_grow, c->w.wt, c->n_imp_local, sp->e_trial, sp->tau);
  else if (apply_rows && c->n_imp_local > 0)
    hipLaunchKernelGGL(k_prj_apply_rows, dim3(nblk(c->n_imp_local, TPB / 64)), dim3(TPB), 0, st, c->d_prj_ptr, c->d_prj_col, c->d_prj_val, x_global_dev,
                       c->d_loc_imp, c->d_grow, c->w.wt, c->n_imp_local, sp->e_trial, sp->tau);
  *order = nullptr;
  if (nsl > 0) {
    u64 *okey = c->d_flags, *okey_alt = c->d_pos; u32 *oval = (u32 *)c->d_flags2, *oval_alt = (u32 *)c->d_pos2;
    if (!c->owner_ready) hipLaunchKernelGGL(k_child_owner, dim3(nblk(nsl)), dim3(TPB), 0, st, c->w, c->d_keys, okey, oval, n0, nsl, c->invalid_key, P, c->pack, c->owner_mode, c->dev.ps.koff);
    SortWork so; so.k_alt = okey_alt; so.v_alt = oval_alt; so.hist = c->d_hist; so.rowtot = c->d_rowtot; so.cap = c->mwalk;
    u64 *sk = okey; u32 *sv = oval;
    device_radix_sort(sk, sv, nsl, 8, so, st, 0, true);      // one stable 8-bit pass (also for a single slot); rowtot[d] = records per destination
    *order = sv;
  }
  c->owner_ready = false;
  HIPCHK(hipGetLastError());
  return SQMC_OK;
}

int sqmc_gpu_shard_pack(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const double *x_global_dev, uint64_t *send_dev, int64_t cap_records,
                        int64_t *send_counts) {
  if (!c || !sp || !send_counts) return fail(SQMC_ERR_BAD_ARG, "null argument");
  hipStream_t st = c->st;
  const long long n0 = c->shard_n0, nsl = c->shard_nslot; const int P = c->shard_n;
  u32 *order;
  int r = shard_bucket(c, sp, x_global_dev, &order); if (r) return r;
  for (int q = 0; q < P; q++) send_counts[q] = 0;
  if (nsl > 0) {
    u32 cnt[256];
    HIPCHK(hipMemcpyAsync(cnt, c->d_rowtot, 256 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    long long nsend = 0;
    for (int q = 0; q < P; q++) { send_counts[q] = cnt[q]; nsend += cnt[q]; }
    if (nsend > cap_records) return fail(SQMC_ERR_SPAWN_OVERFLOW, "send buffer too small for this step's spawns");
    if (nsend > 0) hipLaunchKernelGGL(k_pack_send, dim3(nblk(nsend)), dim3(TPB), 0, st, c->w, order, (u64 *)send_dev, n0, nsend);
  }
  HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(st));
  return SQMC_OK;
}

// phase 3: the records received from all ranks (rank order, creation order inside a rank) become
// the spawned walkers behind the occupied slots; then the usual sort / merge / round / estimate.
static int shard_finish_impl(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const uint64_t *recv_dev, int64_t n_recv, double out[16], bool join,
                             const u64 *self_rec = nullptr, long long self_lo = 0, long long self_hi = 0) {
  if (!c || !sp || !out || n_recv < 0) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  hipStream_t st = c->st;
  const StepP p = step_params(c, sp);
  const long long n0 = c->shard_n0;
  if (n0 + n_recv > c->mwalk) {
    reset_scan_words(c);
    return fail(SQMC_ERR_MWALK, "nwalk>MWALK");
  }
  if (n_recv > 0)
    hipLaunchKernelGGL(k_unpack_recv, dim3(nblk(n_recv)), dim3(TPB), 0, st, c->dev, c->w, (const u64 *)recv_dev, c->d_keys, c->d_vals, n0, (long long)n_recv, c->pack, self_rec, self_lo, self_hi);
  if (n0 + n_recv == 0) {           // an empty shard stays empty this step
    if (join) HIPCHK(hipStreamWaitEvent(st, c->e_join, 0));
    for (int i = 0; i < 16; i++) out[i] = 0.0;
    reset_scan_words(c);
    if (c->psit_shard) {            // still a party to the exchange of the T^-1 partials: nothing to add
      HIPCHK(hipMemsetAsync(c->d_ps_tx, 0, (c->shard_n + 1) * 8, st));
      int rx = psit_shard_exchange(c); if (rx) return rx;
    }
    c->step_no++;
    if (c->comm) {                  // still a party to the all-reduce of the sums
      HIPCHK(hipMemsetAsync(c->d_sc->stats, 0, 16 * 8 + 8 * 8 + 8 * 8, st));       // stats, red and this rank's share of it: nothing to add, no status
      // The collectives of the ranks that hold walkers, in their order: the sums; the coming step's deterministic weights in front of
      // the pipelined head (enqueued before anybody has read the sums); the sums once more if some rank's bucket tail gave up and re-ran.
      const bool head_x = c->pipeline_next && !c->comm2 && c->n_imp > 0 && p.semi;
      c->shard_x_ready = false; c->shard_y_ok = false;
      for (int round = 0; round < 2; round++) {
        if (round == 0 && head_x && !shard_split_allreduce()) {          // one call carries both
          int rp = shard_head_project(c, true, true); if (rp) return rp;
          HIPCHK(hipMemcpyAsync(c->h_sc->red, c->d_xg + c->n_imp, 8 * 8, hipMemcpyDeviceToHost, st));
        } else {
          int rr = comm_allreduce_stats(c); if (rr) return rr;
          HIPCHK(hipMemcpyAsync(c->h_sc, c->d_sc, sizeof(DevScalars), hipMemcpyDeviceToHost, st));
          if (round == 0 && head_x) { int rp = shard_head_project(c, false, true); if (rp) return rp; }
        }
        HIPCHK(hipStreamSynchronize(st));
        const bool again = !err_decode(c->h_sc->red[7]) && fmod(c->h_sc->red[7], 256.0) >= 1.0;
        if (round == 0 && head_x && !again && !err_decode(c->h_sc->red[7])) c->shard_x_ready = true;      // a re-run step redoes its projection
        if (!again) break;
      }
      c->mail_seq++;
      for (int i = 0; i < 7; i++) out[i] = c->h_sc->red[i];
      const int e = err_decode(c->h_sc->red[7]);
      if (e) return fail(e, "another rank stopped the step");
    }
    return SQMC_OK;
  }
  int r = step_tail(c, p, n0, n0 + n_recv, join, out);
  if (r == SQMC_ERR_NO_WALKERS) r = SQMC_OK;      // a shard may legitimately own nothing
  return r;
}
int sqmc_gpu_shard_finish(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const uint64_t *recv_dev, int64_t n_recv, double out[16]) {
  if (c && c->psit_shard && !c->comm) return fail(SQMC_ERR_BAD_ARG, "sharded hf_to_psit without a communicator: finish the step with sqmc_gpu_shard_finish_psit");
  return shard_finish_impl(c, sp, recv_dev, n_recv, out, false);
}
int sqmc_gpu_shard_finish_psit(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const uint64_t *recv_dev, int64_t n_recv, double *reduce_buf_dev,
                               sqmc_allreduce_fn allreduce, void *user, double out[16]) {
  if (!c || !reduce_buf_dev || !allreduce) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (!c->psit_shard) return fail(SQMC_ERR_BAD_ARG, "not a sharded hf_to_psit context (sqmc_gpu_set_hf_to_psit_shard)");
  if (c->comm) return fail(SQMC_ERR_BAD_ARG, "a communicator is attached: the library exchanges the T^-1 partials itself (sqmc_gpu_shard_finish)");
  c->psit_reduce = allreduce; c->psit_reduce_user = user; c->psit_reduce_buf = reduce_buf_dev;
  const int r = shard_finish_impl(c, sp, recv_dev, n_recv, out, false);
  c->psit_reduce = nullptr; c->psit_reduce_user = nullptr; c->psit_reduce_buf = nullptr;
  return r;
}


// ------------------------------------------------------------------ in-library exchange (RCCL over xGMI)
// The three exchanges of a sharded step issued from the library on its own stream, so a step
// costs no Python and no extra host round trips: all-reduce of the deterministic-space vector
// (do_walk.f90:2259-2260), all-to-all of the spawned walkers (mpi_snd_list, mpi_routines.f90:
// 1147-1270 -- here grouped ncclSend/ncclRecv of 32-byte records straight between HBMs), and
// the all-reduce of the seven sums (do_walk.f90:2778-2790).  RCCL is bound at run time from
// the copy already in the process (torch's) or the ROCm one, so single-GPU users never load it.
#define SHARD_ROW(P) ((P) + 2)
struct RcclApi {
  void *lib;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *);
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*CommSplit)(ncclComm_t, int, int, ncclComm_t *, ncclConfig_t *);     // optional (NCCL >= 2.18)
  ncclResult_t (*CommCount)(const ncclComm_t, int *);                                // optional
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*GroupStart)();
  ncclResult_t (*GroupEnd)();
  const char *(*GetErrorString)(ncclResult_t);
};
static RcclApi g_rccl;
static int rccl_bind() {
  if (g_rccl.lib) return SQMC_OK;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  if (const char *over = getenv("SQMC_RCCL_LIB")) h = dlopen(over, RTLD_NOW | RTLD_LOCAL);       // another library with the same entry points (tests: a transport double)
  else for (const char *nm : names) { h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
  if (!h) return fail(SQMC_ERR_UNSUPPORTED, std::string("cannot load RCCL: ") + dlerror());
#define BIND(F) do { *(void **)(&g_rccl.F) = dlsym(h, "nccl" #F); if (!g_rccl.F) return fail(SQMC_ERR_UNSUPPORTED, "RCCL lacks nccl" #F); } while (0)
  BIND(GetUniqueId); BIND(CommInitRank); BIND(CommDestroy); BIND(AllReduce); BIND(AllGather); BIND(Send); BIND(Recv); BIND(GroupStart); BIND(GroupEnd);
  BIND(GetErrorString);
#undef BIND
  *(void **)(&g_rccl.CommSplit) = dlsym(h, "ncclCommSplit");
  *(void **)(&g_rccl.CommCount) = dlsym(h, "ncclCommCount");
  g_rccl.lib = h;
  return SQMC_OK;
}
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail(SQMC_ERR_HIP, std::string(#x) + ": " + g_rccl.GetErrorString(r_)); } while (0)

static void comm_release(sqmc_gpu_ctx *c) {
  if (c->comm2 && g_rccl.lib) g_rccl.CommDestroy(c->comm2);
  if (c->comm && g_rccl.lib) g_rccl.CommDestroy(c->comm);
  c->comm = nullptr; c->comm2 = nullptr;
  hipFree(c->d_xg); hipFree(c->d_send); hipFree(c->d_recv); hipFree(c->d_cnt_mine); hipFree(c->d_cnt_all);
  if (c->h_cnt_all) hipHostFree(c->h_cnt_all);
  c->d_xg = nullptr; c->d_send = c->d_recv = nullptr; c->d_cnt_mine = c->d_cnt_all = nullptr; c->h_cnt_all = nullptr;
}
static int comm_allreduce_stats(sqmc_gpu_ctx *c) {
  // the seven sums every rank needs (do_walk.f90:2778-2790) and the collective status in one call
  NCCLCHK(g_rccl.AllReduce(c->d_sc->redl, c->d_sc->red, 8, ncclDouble, ncclSum, c->comm, c->st));
  return SQMC_OK;
}

// in front of a pipelined head's k_spawn: this rank's deterministic weights into x_global, all-reduced (do_walk.f90:2259-2260)
static int shard_head_project(sqmc_gpu_ctx *c, bool with_sums, bool empty, const FinArgs *fin) {
  hipStream_t st = c->st;
  const size_t nx = (size_t)c->n_imp + (with_sums ? 8 : 0);
  if (empty) HIPCHK(hipMemsetAsync(c->d_xg, 0, nx * 8, st));            // an empty shard adds nothing to either part
  else
    hipLaunchKernelGGL(k_prj_gather_all, dim3(nblk(c->n_imp)), dim3(TPB), 0, st, c->w.wt, c->d_loc_imp, c->d_ginv, c->d_xg, c->n_imp,
                       (const double *)c->d_sc->redl, with_sums ? c->d_xg + c->n_imp : (double *)nullptr, fin ? *fin : FinArgs{}, c->d_sc);
  NCCLCHK(g_rccl.AllReduce(c->d_xg, c->d_xg, nx, ncclDouble, ncclSum, c->comm, st));
  return SQMC_OK;
}

int sqmc_gpu_comm_unique_id(uint8_t id[SQMC_COMM_ID_BYTES]) {
  if (!id) return fail(SQMC_ERR_BAD_ARG, "null argument");
  static_assert(sizeof(ncclUniqueId) <= SQMC_COMM_ID_BYTES, "unique id size");
  int r = rccl_bind(); if (r) return r;
  ncclUniqueId u;
  NCCLCHK(g_rccl.GetUniqueId(&u));
  memset(id, 0, SQMC_COMM_ID_BYTES); memcpy(id, &u, sizeof(u));
  return SQMC_OK;
}

int sqmc_gpu_comm_init(sqmc_gpu_ctx *c, const uint8_t id[SQMC_COMM_ID_BYTES]) {
  if (!c || !id) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (c->shard_n < 1 || !c->d_grow) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_shard_config not called");
  if (c->mwalk <= 0) return fail(SQMC_ERR_BAD_ARG, "no walker arrays");
  int r = rccl_bind(); if (r) return r;
  comm_release(c);
  ncclUniqueId u; memcpy(&u, id, sizeof(u));
  NCCLCHK(g_rccl.CommInitRank(&c->comm, c->shard_n, u, c->shard_rank));
  const int P = c->shard_n;
  c->xch_cap = c->mwalk;             // a rank can neither spawn nor hold more than MWALK walkers
  HIPCHK(hipMalloc(&c->d_xg, (c->n_imp + 9 + 2 * P) * 8));      // + the eight sums that ride behind the weights in a pipelined run; hf_to_psit: 2P row partials
  HIPCHK(hipMalloc(&c->d_send, c->xch_cap * 32)); HIPCHK(hipMalloc(&c->d_recv, c->xch_cap * 32));
  // every rank contributes P send counts + its status + the room behind its walkers (SHARD_ROW words)
  HIPCHK(hipMalloc(&c->d_cnt_mine, SHARD_ROW(P) * 4)); HIPCHK(hipMalloc(&c->d_cnt_all, (size_t)P * SHARD_ROW(P) * 4));
  const size_t cnt_bytes = ((size_t)P * SHARD_ROW(P) + 32) * 4 + 16;
  HIPCHK(hipHostMalloc(&c->h_cnt_all, cnt_bytes, hipHostMallocMapped));     // the P x P send counts + a sequence word: written by the GPU
  memset(c->h_cnt_all, 0, cnt_bytes);
  HIPCHK(hipHostGetDevicePointer((void **)&c->d_cnt_mail, c->h_cnt_all, 0));
  c->cntall_seq = 0;
  // SQMC_SHARD_OVERLAP=1: a second communicator for the all-reduce of the deterministic weights, so that it can run on
  // the side stream beside the spawn path.  Off by default: collectives of two communicators in flight at once are
  // deadlock-prone in NCCL/RCCL unless every rank issues them in one order, and this variant has only met one real rank.
  c->comm2 = nullptr;
  const char *ov = getenv("SQMC_SHARD_OVERLAP");
  if (g_rccl.CommSplit && ov && ov[0] == '1') {
    if (g_rccl.CommSplit(c->comm, 0, c->shard_rank, &c->comm2, nullptr) != ncclSuccess) c->comm2 = nullptr;
  }
  return SQMC_OK;
}

int sqmc_gpu_comm_size(sqmc_gpu_ctx *c, int32_t *nranks) {
  if (!c || !nranks) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (!c->comm) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_comm_init not called");
  int n = c->shard_n;
  if (g_rccl.CommCount) NCCLCHK(g_rccl.CommCount(c->comm, &n));
  *nranks = n;
  return SQMC_OK;
}

// this rank's row of the all-gather: P send counts (the digit totals of the bucketing pass, or zeros), status, room
__global__ void k_fill_counts(const u32 *__restrict__ rowtot, int P, u32 status, u32 room, u32 *__restrict__ mine) {
  for (int k = threadIdx.x; k < P; k += blockDim.x) mine[k] = (rowtot && !status) ? rowtot[k] : 0u;
  if (threadIdx.x == 0) { mine[P] = status; mine[P + 1] = room; }
}
// the P x (P+2) words of the all-gather, posted to pinned host memory (counts, system fence, sequence word)
__global__ void k_post_counts(const u32 *__restrict__ cnt, int n, u32 *mail, u64 seq) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) mail[k] = cnt[k];
  __syncthreads();
  if (threadIdx.x == 0) { __threadfence_system(); *(volatile u64 *)(mail + ((n + 15) / 16) * 16) = seq; }
}

// One sharded MC step with the exchanges inside: out[0..6] are the global sums, out[7..15] local.
// A stop is collective, as the reference's mpi_stop is: a rank that cannot go on (nwalk>MWALK, full send buffer) still
// takes part in every collective up to the all-gather of the counts, which carries its status and the room behind its
// walkers; every rank then returns the same status before any walker moves.  Stops found later (negative diagonal factor,
// broken deterministic space) travel with the all-reduce of the sums.
static int shard_step_impl(sqmc_gpu_ctx *c, const sqmc_step_params *sp, double out[16], double t_us[3]);
int sqmc_gpu_shard_step(sqmc_gpu_ctx *c, const sqmc_step_params *sp, double out[16]) {
  if (!c || !sp || !out) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (!c->comm) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_comm_init not called");
  double t[3] = {0.0, 0.0, 0.0}; t[0] = now_us();
  g_mail_wait_us = &c->sh_us[3];
  const int r = shard_step_impl(c, sp, out, t);
  g_mail_wait_us = nullptr;
  const double t3 = now_us();
  if (t[1] > 0.0 && t[2] > 0.0) { c->sh_us[0] += t[1] - t[0]; c->sh_us[1] += t[2] - t[1]; c->sh_us[2] += t3 - t[2]; c->sh_steps++; }
  return r;
}
int sqmc_gpu_shard_time_split(sqmc_gpu_ctx *c, double us[4], int64_t *steps, int32_t reset) {
  if (!c || !us || !steps) return fail(SQMC_ERR_BAD_ARG, "null argument");
  for (int k = 0; k < 4; k++) us[k] = c->sh_us[k];
  *steps = c->sh_steps;
  if (reset) { for (int k = 0; k < 4; k++) c->sh_us[k] = 0.0; c->sh_steps = 0; }
  return SQMC_OK;
}
static int shard_step_impl(sqmc_gpu_ctx *c, const sqmc_step_params *sp, double out[16], double t_us[3]) {
  hipStream_t st = c->st;
  const int P = c->shard_n, me = c->shard_rank, ROW = SHARD_ROW(P);
  int64_t nch = 0;
  const bool side = (c->comm2 != nullptr) && !c->psit_shard;      // hf_to_psit: one stream (its row partials ride with the weights)
  static const bool diag_side_env = !(getenv("SQMC_SHARD_DIAG_SIDE") && getenv("SQMC_SHARD_DIAG_SIDE")[0] == '0');
  const bool diag_side = !side && diag_side_env && c->st2 != c->st && !c->psit_shard;
  int local = shard_begin_impl(c, sp, c->d_xg, &nch, false, side, diag_side);
  if (local < 0) return local;                     // argument / HIP failures are not walk statuses: nothing collective can be said about them
  const std::string local_msg = local ? g_err : std::string();
  if (local) { c->shard_n0 = c->nwalk; c->shard_nch = 0; c->shard_nslot = 0; }
  t_us[1] = now_us();
  {   // deterministic projection: all-reduce of the weights, then the rows this rank owns
    hipStream_t sx = side ? c->st2 : st;
    if (c->n_imp > 0 && !c->shard_x_used) NCCLCHK(g_rccl.AllReduce(c->d_xg, c->d_xg, (size_t)(c->n_imp + psit_x_extra(c)), ncclDouble, ncclSum, side ? c->comm2 : c->comm, sx));
    if (side) {
      if (c->n_imp_local > 0 && !local)
        hipLaunchKernelGGL(k_prj_apply_rows, dim3(nblk(c->n_imp_local, TPB / 64)), dim3(TPB), 0, sx, c->d_prj_ptr, c->d_prj_col, c->d_prj_val, c->d_xg,
                           c->d_loc_imp, c->d_grow, c->w.wt, c->n_imp_local, sp->e_trial, sp->tau);
      HIPCHK(hipEventRecord(c->e_join, sx));
    }
  }
  // bucket + pack without a host round trip: every spawn slot is packed in destination order (the
  // ones that made no walker sort last and are never sent), the counts stay on the device and go
  // straight into the all-gather that tells every rank who sends how much to whom
  u32 *order = nullptr;
  if (!local) { int r = shard_bucket(c, sp, c->d_xg, &order, !side); if (r) return r; }
  // slots, not children (two per child with fast_heatbath), and slots, not records: the empty ones are packed behind the last rank's
  // and never sent, so the staging buffer is checked against the slot count -- conservative, never a short write
  const long long nsl_l = c->shard_nslot;
  if (!local && nsl_l > c->xch_cap) { local = fail(SQMC_ERR_SPAWN_OVERFLOW, "send buffer too small for this step's spawns"); }
  // the per-destination counts are the digit totals the bucketing pass left in d_rowtot
  const u32 room = (u32)std::min<long long>(c->mwalk - c->shard_n0, 0x7FFFFFFFll);
  if (!local && nsl_l > 0) hipLaunchKernelGGL(k_pack_send, dim3(nblk(nsl_l)), dim3(TPB), 0, st, c->w, order, c->d_send, c->shard_n0, nsl_l, (const u32 *)c->d_rowtot, P, room, c->d_cnt_mine);
  else hipLaunchKernelGGL(k_fill_counts, dim3(1), dim3(256), 0, st, (const u32 *)nullptr, P, (u32)local, room, c->d_cnt_mine);
  NCCLCHK(g_rccl.AllGather(c->d_cnt_mine, c->d_cnt_all, (size_t)ROW, ncclUint32, c->comm, st));
  {
    const u64 qs = ++c->cntall_seq;
    hipLaunchKernelGGL(k_post_counts, dim3(1), dim3(256), 0, st, (const u32 *)c->d_cnt_all, P * ROW, c->d_cnt_mail, qs);
    HIPCHK(hipGetLastError());
    volatile u64 *flag = (volatile u64 *)(c->h_cnt_all + ((P * ROW + 15) / 16) * 16);
    int wr = wait_mail(flag, qs, st);
    if (wr > 0) return mail_fail(wr);
    if (wr < 0) HIPCHK(hipMemcpy(c->h_cnt_all, c->d_cnt_all, (size_t)P * ROW * 4, hipMemcpyDeviceToHost));
  }
  const u32 *all = c->h_cnt_all;
  long long scnt[256], soff[257], roff[257]; soff[0] = roff[0] = 0;
  for (int q = 0; q < P; q++) scnt[q] = all[(size_t)me * ROW + q];
  for (int q = 0; q < P; q++) { soff[q + 1] = soff[q] + scnt[q]; roff[q + 1] = roff[q] + all[(size_t)q * ROW + me]; }
  const long long n_recv = roff[P];
  // the same verdict on every rank: the highest status raised, or nwalk>MWALK if some rank has no room for what it is sent
  int gstat = 0;
  for (int q = 0; q < P; q++) gstat = std::max(gstat, (int)all[(size_t)q * ROW + P]);
  if (!gstat) for (int q = 0; q < P; q++) {
    long long rq = 0; for (int s2 = 0; s2 < P; s2++) rq += all[(size_t)s2 * ROW + q];
    if (rq > (long long)all[(size_t)q * ROW + P + 1]) gstat = SQMC_ERR_MWALK;
  }
  if (gstat) {
    hipStreamSynchronize(st); if (side || diag_side) hipStreamSynchronize(c->st2);
    reset_scan_words(c);
    if (local == gstat) return fail(gstat, local_msg.empty() ? g_err : local_msg);
    return fail(gstat, gstat == SQMC_ERR_MWALK ? "nwalk>MWALK (on some rank)" : "another rank stopped the step");
  }
  // the walkers themselves, HBM to HBM; records from rank q land at roff[q] (rank order,
  // creation order inside a rank: the order the merge rules see, do_walk.f90:5866-6083)
  NCCLCHK(g_rccl.GroupStart());
  for (int q = 0; q < P; q++) {
    if (q == me) continue;
    if (scnt[q] > 0) NCCLCHK(g_rccl.Send(c->d_send + 4 * soff[q], (size_t)(4 * scnt[q]), ncclUint64, q, c->comm, st));
    const long long rc = roff[q + 1] - roff[q];
    if (rc > 0) NCCLCHK(g_rccl.Recv(c->d_recv + 4 * roff[q], (size_t)(4 * rc), ncclUint64, q, c->comm, st));
  }
  NCCLCHK(g_rccl.GroupEnd());
  t_us[2] = now_us();
  return shard_finish_impl(c, sp, (const uint64_t *)c->d_recv, n_recv, out, side || (diag_side && c->shard_n0 > 0), c->d_send + 4 * soff[me], roff[me], roff[me] + scnt[me]);
}

int sqmc_gpu_shard_run(sqmc_gpu_ctx *c, sqmc_popctl *pc, int64_t nsteps, double *stats, double totals[16]) {
  return run_steps(c, pc, nsteps, stats, totals, sqmc_gpu_shard_step);
}

// ------------------------------------------------------------------ hf_to_psit over ranks
// do_walk.f90:1808-1886 (set-up), 2272-2288 and 2304-2320 (before the merge), 2394-2442 (T^-1 after it), 2444-2462 and 2701-2722 (the
// C(T) loops over the local share).  psit_kernels.h has the device side; DESIGN.md section 4b the exchanges and the sum order.
int sqmc_gpu_set_hf_to_psit_shard(sqmc_gpu_ctx *c, int64_t n_ct_local, const int64_t *ct_index, const double *diag_elems, int64_t n_psit_local,
                                  const int64_t *psit_slot, const int64_t *psit_mask, int64_t n_psit, const double *cdet_psi_t, int32_t sum_order) {
  abandon_head(c);
  if (!c || n_ct_local < 0 || n_psit_local < 0 || n_psit < 1 || !cdet_psi_t || (n_ct_local > 0 && (!ct_index || !diag_elems)) ||
      (n_psit_local > 0 && (!psit_slot || !psit_mask))) return fail(SQMC_ERR_BAD_ARG, "bad argument");
  if (c->htab.sys_type == 3) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit is not built for the Hubbard model in plane waves (hubbardk)");
  if (c->mwalk <= 0) return fail(SQMC_ERR_BAD_ARG, "context has no walker arrays (mwalk=0)");
  if (c->shard_n < 1 || !c->d_grow) return fail(SQMC_ERR_BAD_ARG, "call sqmc_gpu_shard_config before sqmc_gpu_set_hf_to_psit_shard");
  if (c->dev.hb.on) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit with proposal_method fast_heatbath is not built");
  if (c->dev.cs.on) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit with proposal_method CauchySchwarz is not built");
  if (c->htab.sys_type == 2) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit is not built for the Hubbard model");
  if (!c->d_ct_up || c->n_ct < 1) return fail(SQMC_ERR_BAD_ARG, "set the (global) C(T) table first");
  if (!c->d_prj_ptr || c->n_imp < 1) return fail(SQMC_ERR_BAD_ARG, "set the (global) deterministic-space matrix first");
  if (sum_order != 0 && sum_order != 1) return fail(SQMC_ERR_BAD_ARG, "sum_order must be 0 (left to right) or 1 (64-ary tree)");
  if (n_psit - 1 > PSIT_MAXTERMS || n_ct_local > PSIT_MAXTERMS) return fail(SQMC_ERR_UNSUPPORTED, "trial wave function or C(T) share longer than 64^3 determinants: the tree sums have three levels");
  if (n_ct_local > c->n_ct || n_psit_local > n_psit) return fail(SQMC_ERR_BAD_ARG, "a share is longer than the global table");
  if (cdet_psi_t[0] == 0.0) return fail(SQMC_ERR_BAD_ARG, "cdet_psi_t(1) = 0");
  for (long long i = 0; i < n_ct_local; i++)
    if (ct_index[i] < 1 || ct_index[i] > c->n_ct || (i && ct_index[i] <= ct_index[i - 1])) return fail(SQMC_ERR_BAD_ARG, "ct_index must be increasing 1-based positions in the C(T) list");
  std::vector<int> loc(n_psit_local + 1), of(n_ct_local + 1, -1);
  for (long long k = 0; k < n_psit_local; k++) {
    const long long q = psit_slot[k] - 1;
    if (q < 0 || q >= n_ct_local || (k && q <= loc[k - 1])) return fail(SQMC_ERR_BAD_ARG, "psit_slot must be increasing 1-based positions in this rank's C(T) share");
    if (psit_mask[k] < 1 || psit_mask[k] > n_psit || (k && psit_mask[k] <= psit_mask[k - 1])) return fail(SQMC_ERR_BAD_ARG, "psit_mask must be increasing 1-based indices of Psi_T (label order)");
    loc[k] = (int)q; of[q] = (int)k;
  }
  // iown_first = iown_psit1: the first state is C(T)'s and Psi_T's first determinant (host.psit_tables), at the head of its owner's share
  const bool own_first = n_ct_local > 0 && ct_index[0] == 1;
  if (own_first != (n_psit_local > 0 && psit_mask[0] == 1) || (own_first && loc[0] != 0))
    return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit: the first determinant of Psi_T must be the first determinant of C(T), at slot 1 of its owner's share");
  u64 total = 0;
  { auto choose = [&](int n_, int k_) -> long double { long double r = 1; for (int q = 1; q <= k_; q++) r = r * (n_ - k_ + q) / q; return r; };
    total = (u64)(choose(c->htab.norb, c->htab.nup) * choose(c->htab.norb, c->htab.ndn) + 0.5L); }
  if (!c->base_key_bits) c->base_key_bits = c->key_bits;
  if (c->base_key_bits + 1 > 62) return fail(SQMC_ERR_UNSUPPORTED, "determinant space too large for the hf_to_psit sort key");
  psit_off(c);
  // this rank's rows of the global C(T) table: determinants (the upload checks them), e_loc_num / den
  const long long n_ct = c->n_ct, P = c->shard_n;
  std::vector<u64> gu(n_ct), gd(n_ct); std::vector<double> gn(n_ct), gdn(n_ct);
  HIPCHK(hipMemcpy(gu.data(), c->d_ct_up, n_ct * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(gd.data(), c->d_ct_dn, n_ct * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(gn.data(), c->d_ct_num, n_ct * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(gdn.data(), c->d_ct_den, n_ct * 8, hipMemcpyDeviceToHost));
  c->ps_ct_up.assign(n_ct_local, 0); c->ps_ct_dn.assign(n_ct_local, 0);
  std::vector<double> num(n_ct_local + 1, 0.0), den(n_ct_local + 1, 0.0), cl(n_psit_local + 1, 0.0);
  for (long long i = 0; i < n_ct_local; i++) { const long long g = ct_index[i] - 1; c->ps_ct_up[i] = gu[g]; c->ps_ct_dn[i] = gd[g]; num[i] = gn[g]; den[i] = gdn[g]; }
  for (long long k = 0; k < n_psit_local; k++) cl[k] = cdet_psi_t[psit_mask[k] - 1];
  hipFree(c->d_ps_loc); hipFree(c->d_ps_of); hipFree(c->d_ps_impof); hipFree(c->d_ps_c); hipFree(c->d_ps_diag); hipFree(c->d_ps_dwct); hipFree(c->d_ps_dwps);
  hipFree(c->d_ps_dwimp); hipFree(c->d_ps_p2); hipFree(c->d_ps_part); hipFree(c->d_ps_raw); hipFree(c->d_ps_num); hipFree(c->d_ps_den); hipFree(c->d_ps_tx);
  c->d_ps_loc = c->d_ps_of = c->d_ps_impof = nullptr; c->d_ps_c = c->d_ps_diag = c->d_ps_dwct = c->d_ps_dwps = c->d_ps_dwimp = c->d_ps_p2 = c->d_ps_part = c->d_ps_raw = nullptr;
  c->d_ps_num = c->d_ps_den = c->d_ps_tx = nullptr;
  const long long nc1 = n_ct_local + 1, np1 = n_psit_local + 1;      // (+1: no zero-length allocation for an empty share)
  HIPCHK(hipMalloc(&c->d_ps_raw, np1 * 8)); HIPCHK(hipMalloc(&c->d_ps_loc, np1 * 4)); HIPCHK(hipMalloc(&c->d_ps_of, nc1 * 4)); HIPCHK(hipMalloc(&c->d_ps_impof, nc1 * 4));
  HIPCHK(hipMalloc(&c->d_ps_c, np1 * 8)); HIPCHK(hipMalloc(&c->d_ps_diag, nc1 * 8)); HIPCHK(hipMalloc(&c->d_ps_dwct, nc1 * 8)); HIPCHK(hipMalloc(&c->d_ps_dwps, np1 * 8));
  HIPCHK(hipMalloc(&c->d_ps_dwimp, (c->n_imp + 1) * 8)); HIPCHK(hipMalloc(&c->d_ps_p2, ((n_ct_local + 4095) / 4096 + 1) * 8)); HIPCHK(hipMalloc(&c->d_ps_part, (size_t)PSIT_FB * NSTAT * 8));
  HIPCHK(hipMalloc(&c->d_ps_num, nc1 * 8)); HIPCHK(hipMalloc(&c->d_ps_den, nc1 * 8)); HIPCHK(hipMalloc(&c->d_ps_tx, (P + 1) * 8));
  HIPCHK(hipMemcpy(c->d_ps_loc, loc.data(), np1 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(c->d_ps_of, of.data(), nc1 * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_ps_impof, 0xFF, nc1 * 4));               // filled by the upload
  HIPCHK(hipMemcpy(c->d_ps_c, cl.data(), np1 * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_ps_diag, 0, nc1 * 8)); if (n_ct_local > 0) HIPCHK(hipMemcpy(c->d_ps_diag, diag_elems, n_ct_local * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->d_ps_num, num.data(), nc1 * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(c->d_ps_den, den.data(), nc1 * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(c->d_ps_tx, 0, (P + 1) * 8));
  PsitArgs &a = c->psit; memset(&a, 0, sizeof(a));
  a.n_ct = n_ct_local; a.n_psit = n_psit_local; a.n_imp = c->n_imp; a.loc_psit = c->d_ps_loc; a.cdet = c->d_ps_c; a.diag = c->d_ps_diag; a.psit_of = c->d_ps_of;
  a.imp_of = c->d_ps_impof; a.cnum = c->d_ps_num; a.cden = c->d_ps_den; a.dw_ct = c->d_ps_dwct; a.dw_ps = c->d_ps_dwps; a.dw_imp = c->d_ps_dwimp; a.p2 = c->d_ps_p2;
  a.n_perm = 0; a.seq = sum_order == 0 ? 1 : 0;
  a.own_first = own_first ? 1 : 0; a.c1 = cdet_psi_t[0]; a.tx = c->d_ps_tx; a.shard_P = (int)P; a.shard_me = c->shard_rank;
  c->dev.ps.koff = total; c->dev.ps.hkey = c->d_ct_hkey; c->dev.ps.hmask = c->ct_mask; c->dev.ps.first_up = gu[0]; c->dev.ps.first_dn = gd[0];
  c->dev.ps.n_ct = n_ct_local; c->dev.ps.own_first = a.own_first;
  c->key_bits = c->base_key_bits + 1; c->invalid_key = (1ull << c->key_bits) - 1ull;
  c->pack = (c->key_bits <= 32 && !getenv("SQMC_FORCE_UNPACKED")) ? 1 : 0;
  c->psit_on = true; c->psit_shard = true; c->nwalk = 0;           // walkers are uploaded anew: this rank's share of C(T) first
  return SQMC_OK;
}

// before the merge, behind the all-reduce of x_global: the deterministic-space rows this rank owns (no E_T term), the first column over its
// share with w_1 = x_global(1), the first rows on the owner (partials of all ranks in rank order), then the update slot by slot (2304-2320)
static int psit_shard_project(sqmc_gpu_ctx *c, const sqmc_step_params *sp, const double *xg) {
  hipStream_t st = c->st;
  const PsitArgs &a = c->psit;
  if (c->n_imp_local > 0)
    hipLaunchKernelGGL(k_psit_imp_rows, dim3(nblk(c->n_imp_local, TPB / 64)), dim3(TPB), 0, st, prj_pre(c, xg, a.dw_imp, true));
  if (a.n_ct > 0) hipLaunchKernelGGL(k_psit_ct_col, dim3(nblk(a.n_ct)), dim3(TPB), 0, st, a, (const double *)c->w.wt, xg);
  hipLaunchKernelGGL(k_psit_rows_fin_shard, dim3(1), dim3(TPB), 0, st, a, xg, sp->tau, sp->e_trial);
  if (a.n_ct > 0) hipLaunchKernelGGL(k_psit_apply, dim3(nblk(a.n_ct)), dim3(TPB), 0, st, a, c->w.wt, sp->tau, sp->e_trial);
  HIPCHK(hipGetLastError());
  return SQMC_OK;
}
// the P + 1 doubles of the T^-1 exchange, summed over ranks in place: RCCL with a communicator, else the caller's all-reduce
static int psit_shard_exchange(sqmc_gpu_ctx *c) {
  hipStream_t st = c->st;
  const size_t n = (size_t)c->shard_n + 1;
  if (c->comm) { NCCLCHK(g_rccl.AllReduce(c->d_ps_tx, c->d_ps_tx, n, ncclDouble, ncclSum, c->comm, st)); return SQMC_OK; }
  if (!c->psit_reduce) return fail(SQMC_ERR_BAD_ARG, "sharded hf_to_psit without a communicator: finish the step with sqmc_gpu_shard_finish_psit");
  HIPCHK(hipMemcpyAsync(c->psit_reduce_buf, c->d_ps_tx, n * 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->psit_reduce(c->psit_reduce_buf, (int64_t)n, c->psit_reduce_user) != 0) return fail(SQMC_ERR_BAD_ARG, "the caller's all-reduce of the T^-1 partials failed");
  HIPCHK(hipMemcpyAsync(c->d_ps_tx, c->psit_reduce_buf, n * 8, hipMemcpyDeviceToDevice, st));
  return SQMC_OK;
}
static int psit_shard_tinv(sqmc_gpu_ctx *c, const double *ps_raw) {
  hipLaunchKernelGGL(k_psit_tinv_part, dim3(1), dim3(64), 0, c->st, c->psit, ps_raw, c->d_ps_tx);
  HIPCHK(hipGetLastError());
  return psit_shard_exchange(c);
}
