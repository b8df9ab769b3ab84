// abi_rdm2.inc -- C-ABI entry point of the two-body reduced density matrix (inside extern "C"); kernels in rdm2_kernels.h, compiled in
// rdm2_device.hip and launched through rdm2_launch.h; the host arithmetic in rdm2_plan.h.  Textually included by sqmc_gpu.hip behind abi_rdm.inc (RdmList, rdm_list_build, rdm_refuse_basis).

// tools/rdm2_time.py: HIP events around the kernels of a block (SQMC_RDM2_TIME set when the library first runs one)
static bool rdm2_timed() { static const bool on = getenv("SQMC_RDM2_TIME") != nullptr; return on; }

// one spin block of a built list into d_out (norb^4 doubles on the device, every entry written)
static int rdm2_block_dev(sqmc_gpu_ctx *c, const char *who, const RdmList &L, const Rdm2Shape &sh, double *d_out) {
  hipStream_t st = c->st;
  const int norb = sh.norb;
  const size_t n4 = (size_t)norb * norb * norb * norb;
  c->rdm2_ms[sh.kind] = 0.0; c->rdm2_records[sh.kind] = 0;
  HIPDOOR(who, hipMemsetAsync(d_out, 0, n4 * 8, st));
  if (sh.R == 0) { HIPDOOR(who, hipStreamSynchronize(st)); return SQMC_OK; }      // no pair of electrons of this kind: all zeros, nothing launched
  const long long nrec = L.n * (long long)sh.R;
  DevScratch s(st);
  EventMarks ev(rdm2_timed(), 2);
  u64 *sK = s.take<u64>(nrec); u32 *sP = s.take<u32>(nrec); double *sV = s.take<double>(nrec); u32 *start = s.take<u32>((size_t)sh.npairs + 1);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, ev.mark(st));
  {
    DevScratch w(st);                    // the unsorted records and the sort's scratch: gone before the Gram matrix is allocated
    u64 *key = w.take<u64>(nrec), *kalt = w.take<u64>(nrec), *K = w.take<u64>(nrec); u32 *idx = w.take<u32>(nrec), *ialt = w.take<u32>(nrec), *P = w.take<u32>(nrec);
    double *V = w.take<double>(nrec); u32 *hist = w.take<u32>((size_t)((nrec + RS_TILE - 1) / RS_TILE) * RS_MAX_RADIX), *rt = w.take<u32>(RS_MAX_RADIX);
    if (!w.ok()) return hip_fail(who, w.err());
    rdm2_launch_emit(st, c->dev.binom, L.su, L.sd, L.sc, L.n, sh, key, idx, K, P, V);
    SortWork so; so.k_alt = kalt; so.v_alt = ialt; so.hist = hist; so.rowtot = rt; so.cap = nrec;
    if (sh.oneword) device_radix_sort(key, idx, nrec, sh.kbits + sh.pbits, so, st);
    else {
      device_radix_sort(key, idx, nrec, sh.kbits, so, st);
      rdm2_launch_pairkeys(st, idx, P, nrec, key);
      device_radix_sort(key, idx, nrec, sh.pbits, so, st);
    }
    rdm2_launch_sorted(st, idx, K, P, V, nrec, sK, sP, sV);
    rdm2_launch_colstart(st, sP, nrec, sh.npairs, start);
    HIPDOOR(who, hipGetLastError());
  }
  std::vector<uint32_t> hstart((size_t)sh.npairs + 1), hcol;
  HIPDOOR(who, hipMemcpyAsync(hstart.data(), start, hstart.size() * 4, hipMemcpyDeviceToHost, st)); HIPDOOR(who, hipStreamSynchronize(st));
  long long nheavy = 0;
  rdm2_column_order(hstart, hcol, &nheavy);
  const long long m = (long long)hcol.size(), nent = m * (m + 1) / 2, eh = nheavy * (nheavy + 1) / 2;
  if (m < 1 || hstart[sh.npairs] != (uint32_t)nrec) return fail(SQMC_ERR_HIP, std::string(who) + ": the sorted records do not add up");
  u32 *col = s.take<u32>(m); double *gram = s.take<double>(nent);
  if (!s.ok()) return hip_fail(who, s.err());
  HIPDOOR(who, hipMemcpy(col, hcol.data(), m * 4, hipMemcpyHostToDevice));
  rdm2_launch_gram(st, sK, sV, start, col, eh, nent, gram);
  rdm2_launch_expand(st, gram, col, nent, sh.kind, norb, d_out);
  HIPDOOR(who, hipGetLastError()); HIPDOOR(who, ev.mark(st)); HIPDOOR(who, hipStreamSynchronize(st));
  ev.add(&c->rdm2_ms[sh.kind]);
  c->rdm2_records[sh.kind] = nrec;
  return SQMC_OK;
}

static int rdm2_door(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, int32_t blocks,
                     double *rdm_aa, double *rdm_bb, double *rdm_ab) {
  const char *who = "sqmc_gpu_hci_2rdm";
  if (!c || !var_up || !var_dn || !coeffs || n_var < 1) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2rdm: bad argument");
  if (blocks < 1 || blocks > 7) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2rdm: blocks must be 1 (aa), 2 (bb), 4 (ab) or a sum of them");
  double *dst[3] = {rdm_aa, rdm_bb, rdm_ab};
  for (int k = 0; k < 3; k++) if ((blocks >> k & 1) && !dst[k]) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_hci_2rdm: a requested block has a null pointer");
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
  if ((rc = rdm_list_build(c, who, n_var, var_up, var_dn, coeffs, L)) != SQMC_OK) return rc;
  const size_t n4 = (size_t)norb * norb * norb * norb;
  std::vector<double> host[3];           // declared ahead of s: s waits for the stream before a copy's target goes
  DevScratch s(c->st);
  for (int k = 0; k < 3; k++) {
    if (!(blocks >> k & 1)) continue;
    double *d_out = s.take<double>(n4);
    if (!s.ok()) return hip_fail(who, s.err());
    if ((rc = rdm2_block_dev(c, who, L, sh[k], d_out)) != SQMC_OK) return rc;
    host[k].resize(n4);
    HIPDOOR(who, hipMemcpy(host[k].data(), d_out, n4 * 8, hipMemcpyDeviceToHost));
    s.drop(d_out);
  }
  for (int k = 0; k < 3; k++) if (blocks >> k & 1) memcpy(dst[k], host[k].data(), n4 * 8);      // only finished blocks reach the caller, and only when all are
  return SQMC_OK;
}
// the staging arrays (norb^4 doubles per block: 134 MB at 64 orbitals) and the column tables are std::vectors: a host allocation that
// fails is an error return like any other, and by then nothing has reached the caller's arrays
int sqmc_gpu_hci_2rdm(sqmc_gpu_ctx *c, int64_t n_var, const uint64_t *var_up, const uint64_t *var_dn, const double *coeffs, int32_t blocks,
                      double *rdm_aa, double *rdm_bb, double *rdm_ab) {
  try { return rdm2_door(c, n_var, var_up, var_dn, coeffs, blocks, rdm_aa, rdm_bb, rdm_ab); }
  catch (const std::bad_alloc &) { return fail(SQMC_ERR_HIP, "sqmc_gpu_hci_2rdm: out of host memory"); }
}
// milliseconds the kernels of each block of the last 2-RDM call took (0 unless SQMC_RDM2_TIME was set when the library first ran one)
// and the records of each block; three entries each, aa, bb, ab; not part of the ABI
int sqmc_gpu_debug_rdm2_ms(sqmc_gpu_ctx *c, double *ms, int64_t *records) {
  if (!c || !ms || !records) return SQMC_ERR_BAD_ARG;
  for (int k = 0; k < 3; k++) { ms[k] = c->rdm2_ms[k]; records[k] = c->rdm2_records[k]; }
  return SQMC_OK;
}
