// abi_tdm.inc -- C-ABI entry points of the one- and two-body transition density matrices of two coefficient vectors over one
// determinant list (inside extern "C"); kernels in tdm_kernels.h, compiled in tdm_device.hip and launched through tdm_launch.h (the
// records' emit, sort and column starts through rdm2_launch.h); the host arithmetic is rdm2_plan.h's, unchanged.  Textually included
// by sqmc_gpu.hip behind abi_rdm2.inc (RdmList, rdm_list_build with its second coefficient array, rdm_refuse_basis, rdm2_timed).
static_assert(TDM1_T == RDM_T && TDM1_CHUNK == RDM_CHUNK, "the one-body transition kernel keeps the 1-RDM's block and chunk");

// one spin block of a built list (L.sc = ket, L.sc2 = bra) into d_out (norb^4 doubles on the device, every entry written): the
// pipeline of rdm2_block_dev with a second value column
static int tdm2_block_dev(sqmc_gpu_ctx *c, const char *who, const RdmList &L, const Rdm2Shape &sh, double *d_out) {
  hipStream_t st = c->st;
  const int norb = sh.norb;
  const size_t n4 = (size_t)norb * norb * norb * norb;
  c->rdm2_ms[sh.kind] = 0.0; c->rdm2_records[sh.kind] = 0;
  HIPDOOR(who, hipMemsetAsync(d_out, 0, n4 * 8, st));
  if (sh.R == 0) { HIPDOOR(who, hipStreamSynchronize(st)); return SQMC_OK; }      // no pair of electrons of this kind: all zeros, nothing launched
  const long long nrec = L.n * (long long)sh.R;
  DevScratch s(st);
  EventMarks ev(rdm2_timed(), 2);
  u64 *sK = s.take<u64>(nrec); u32 *sP = s.take<u32>(nrec); double *sU = s.take<double>(nrec), *sW = s.take<double>(nrec); u32 *start = s.take<u32>((size_t)sh.npairs + 1);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, ev.mark(st));
  {
    DevScratch w(st);                    // the unsorted records and the sort's scratch: gone before the Gram matrix is allocated
    u64 *key = w.take<u64>(nrec), *kalt = w.take<u64>(nrec), *K = w.take<u64>(nrec); u32 *idx = w.take<u32>(nrec), *ialt = w.take<u32>(nrec), *P = w.take<u32>(nrec);
    double *U = w.take<double>(nrec), *W = w.take<double>(nrec); u32 *hist = w.take<u32>((size_t)((nrec + RS_TILE - 1) / RS_TILE) * RS_MAX_RADIX), *rt = w.take<u32>(RS_MAX_RADIX);
    if (!w.ok()) return hip_fail(who, w.err());
    rdm2_launch_emit(st, c->dev.binom, L.su, L.sd, L.sc, L.n, sh, key, idx, K, P, W);
    tdm_launch_bra(st, L.sc2, L.n, sh, U);
    SortWork so; so.k_alt = kalt; so.v_alt = ialt; so.hist = hist; so.rowtot = rt; so.cap = nrec;
    if (sh.oneword) device_radix_sort(key, idx, nrec, sh.kbits + sh.pbits, so, st);
    else {
      device_radix_sort(key, idx, nrec, sh.kbits, so, st);
      rdm2_launch_pairkeys(st, idx, P, nrec, key);
      device_radix_sort(key, idx, nrec, sh.pbits, so, st);
    }
    tdm_launch_sorted(st, idx, K, P, U, W, nrec, sK, sP, sU, sW);
    rdm2_launch_colstart(st, sP, nrec, sh.npairs, start);
    HIPDOOR(who, hipGetLastError());
  }
  std::vector<uint32_t> hstart((size_t)sh.npairs + 1), hcol;
  HIPDOOR(who, hipMemcpyAsync(hstart.data(), start, hstart.size() * 4, hipMemcpyDeviceToHost, st)); HIPDOOR(who, hipStreamSynchronize(st));
  long long nheavy = 0;
  rdm2_column_order(hstart, hcol, &nheavy);
  const long long m = (long long)hcol.size(), nent = m * (m + 1) / 2, eh = nheavy * (nheavy + 1) / 2;
  if (m < 1 || hstart[sh.npairs] != (uint32_t)nrec) return fail(SQMC_ERR_HIP, std::string(who) + ": the sorted records do not add up");
  u32 *col = s.take<u32>(m); double *gram = s.take<double>(2 * nent);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpy(col, hcol.data(), m * 4, hipMemcpyHostToDevice));
  tdm_launch_gram(st, sK, sU, sW, start, col, eh, nent, gram);
  tdm_launch_expand(st, gram, col, nent, sh.kind, norb, d_out);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st)); HIPDOOR(who, hipStreamSynchronize(st));
  ev.add(&c->rdm2_ms[sh.kind]);
  c->rdm2_records[sh.kind] = nrec;
  return SQMC_OK;
}

static int tdm2_door(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket, int32_t blocks,
                     double *tdm_aa, double *tdm_bb, double *tdm_ab) {
  const char *who = "sqmc_gpu_hci_2tdm";
  if (!c || !var_up || !var_dn || !bra || !ket || n_var < 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2tdm: bad argument");
  if (blocks < 1 || blocks > 7) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2tdm: blocks must be 1 (aa), 2 (bb), 4 (ab) or a sum of them");
  double *dst[3] = {tdm_aa, tdm_bb, tdm_ab};
  for (int k = 0; k < 3; k++) if ((blocks >> k & 1) && !dst[k]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2tdm: a requested block has a null pointer");
  int rc = rdm_refuse_basis(c, who);
  if (rc != SQMC_OK) return rc;
  const int norb = c->htab.norb;
  for (int k = 0; k < 3; k++) { c->rdm2_ms[k] = 0.0; c->rdm2_records[k] = 0; }
  Rdm2Shape sh[3];
  for (int k = 0; k < 3; k++) {
    sh[k] = rdm2_shape(k, norb, c->htab.nup, c->htab.ndn);
    if (!(blocks >> k & 1)) continue;
    if (!sh[k].fits) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": the (N-2)-electron key space of block " + (k == 0 ? "aa" : k == 1 ? "bb" : "ab") + " needs more than 64 bits");
    if ((unsigned __int128)n_var * (unsigned)sh[k].R >= 0xFFFFFFFFull) return fail(SQMC_ERR_UNSUPPORTED, std::string(who) + ": a block with 2^32 - 1 records or more");
  }
  RdmList L(c->st);
  if ((rc = rdm_list_build(c, who, n_var, var_up, var_dn, ket, L, bra)) != SQMC_OK) return rc;
  const size_t n4 = (size_t)norb * norb * norb * norb;
  std::vector<double> host[3];           // declared ahead of s: s waits for the stream before a copy's target goes
  DevScratch s(c->st);
  for (int k = 0; k < 3; k++) {
    if (!(blocks >> k & 1)) continue;
    double *d_out = s.take<double>(n4);
    if (!s.ok()) return hip_fail(who, s.err());
    if ((rc = tdm2_block_dev(c, who, L, sh[k], d_out)) != SQMC_OK) return rc;
    host[k].resize(n4);
    HIPDOOR(who, hipMemcpy(host[k].data(), d_out, n4 * 8, hipMemcpyDeviceToHost));
    s.drop(d_out);
  }
  for (int k = 0; k < 3; k++) if (blocks >> k & 1) memcpy(dst[k], host[k].data(), n4 * 8);      // only finished blocks reach the caller, and only when all are
  return SQMC_OK;
}
int sqmc_gpu_hci_2tdm(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket, int32_t blocks,
                      double *tdm_aa, double *tdm_bb, double *tdm_ab) {
  try { return tdm2_door(c, n_var, var_up, var_dn, bra, ket, blocks, tdm_aa, tdm_bb, tdm_ab); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_hci_2tdm: out of host memory"); }
}

static int tdm1_door(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket,
                     const int32_t *orbital_symmetries, double *tdm) {
  const char *who = "sqmc_gpu_hci_1tdm";
  if (!c || !var_up || !var_dn || !bra || !ket || !tdm || n_var <= 0) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1tdm: bad argument");
  int rc = rdm_refuse_basis(c, who);
  if (rc != SQMC_OK) return rc;
  const int norb = c->htab.norb;
  std::vector<unsigned char> sym(norb);
  if (orbital_symmetries)
    for (int i = 0; i < norb; i++) {
      if (orbital_symmetries[i] < 0 || orbital_symmetries[i] > 255) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_1tdm: an orbital symmetry label outside 0..255");
      sym[i] = (unsigned char)orbital_symmetries[i];
    }
  RdmList L(c->st);
  if ((rc = rdm_list_build(c, who, n_var, var_up, var_dn, ket, L, bra)) != SQMC_OK) return rc;
  const int nchunks = (int)((L.n + TDM1_CHUNK - 1) / TDM1_CHUNK);
  std::vector<double> host((size_t)norb * norb);      // declared ahead of s: s waits for the stream before the copy's target goes
  DevScratch s(c->st);
  double *d_tdm = s.take<double>((size_t)norb * norb), *part = s.take<double>((size_t)nchunks * norb * (norb + 1) * 2);
  unsigned char *dsym = orbital_symmetries ? s.take<unsigned char>(norb) : nullptr;
  if (!s.ok()) return hip_fail(who, s.err());
  if (dsym) HIPDOOR(who, hipMemcpy(dsym, sym.data(), norb, hipMemcpyHostToDevice));
  EventMarks ev(rdm_timed(), 2);
  c->rdm_var_ms = 0.0;
  HIPDOOR(who, ev.mark(c->st));
  tdm_launch_one(c->st, c->dev, L.su, L.sd, L.sc2, L.sc, L.n, L.skey, norb, dsym, part, d_tdm);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(c->st)); HIPDOOR(who, hipStreamSynchronize(c->st));
  ev.add(&c->rdm_var_ms);
  HIPDOOR(who, hipMemcpy(host.data(), d_tdm, host.size() * 8, hipMemcpyDeviceToHost));
  memcpy(tdm, host.data(), host.size() * 8);      // only a finished matrix reaches the caller
  return SQMC_OK;
}
// the label and staging arrays are std::vectors: a host allocation that fails is an error return like any other
int sqmc_gpu_hci_1tdm(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *bra, const double *ket,
                      const int32_t *orbital_symmetries, double *tdm) {
  try { return tdm1_door(c, n_var, var_up, var_dn, bra, ket, orbital_symmetries, tdm); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_hci_1tdm: out of host memory"); }
}
