// heatbath_setup.inc -- the tables of the efficient heat-bath proposal built by the library itself: setup_efficient_heatbath for
// run_type /= hci (chemistry.f90:1002-1225), check_heatbath_unbiased (9330-9375), setup_alias_rk / _real (more_tools.f90:5603-5722).
// Textually included by sqmc_gpu.hip inside its extern "C" block.
//
// The |H_ijkl| of all orbital quadruples come from the device (the batch kernel behind sqmc_gpu_hamiltonian_chem_batch on
// two-electron determinants, as the reference calls hamiltonian_chem with nosign); the partial sums, their normalisation and the
// alias tables are built on the host in the reference's loop order -- the four-index tables are accumulated and normalised in
// single precision exactly where the reference's `real(...)` conversions stand, including the second normalisation a same-spin
// slice sees when its electron pair comes round as (j, i).  The tables are then installed with sqmc_gpu_set_heatbath_tables and
// kept on the host in the reference's (column-major, 1-based) layout for sqmc_gpu_get_heatbath_tables.

extern "C++" {
static long long hbs_c2i(int i, int j) { return i > j ? ((long long)i * (i - 1)) / 2 + j : ((long long)j * (j - 1)) / 2 + i; }      // combine_2_indices, chemistry.f90:9138-9150
template <class T>
static void hbs_alias(int K, const T *pdf, int *smaller, int *larger, int *J, T *q) {      // more_tools.f90:5603-5722; J, q, pdf: K consecutive entries, 1-based values in J
  int n_s = 0, n_l = 0;
  for (int i = 1; i <= K; i++) {
    J[i - 1] = i; q[i - 1] = (T)K * pdf[i - 1];
    if (q[i - 1] < (T)1.0) smaller[n_s++] = i; else larger[n_l++] = i;
  }
  while (n_s > 0 && n_l > 0) {
    const int small = smaller[n_s - 1], large = larger[n_l - 1];
    J[small - 1] = large;
    q[large - 1] = q[large - 1] + q[small - 1] - (T)1.0;
    if (q[large - 1] < (T)1.0) { smaller[n_s - 1] = large; n_l--; } else n_s--;
  }
}
struct HbHost {          // host copies in the ABI's layout (freed by sqmc_gpu_finalize)
  std::vector<double> one, two, three_same, three_opp, q3_same, q3_opp, htot_same, htot_opp;
  std::vector<int32_t> j3_same, j3_opp, j4_same, j4_opp;
  std::vector<float> four_same, four_opp, q4_same, q4_opp;
  long long size_same, size_opp; int norb, unbiased, n_orb_uniq_sym;
};
}   // extern "C++"

int sqmc_gpu_setup_efficient_heatbath(sqmc_gpu_ctx *c, int32_t *is_heatbath_unbiased) {
  abandon_head(c);
  if (!c) return fail(SQMC_ERR_BAD_ARG, "null ctx");
  if (c->htab.sys_type != 0) return fail(SQMC_ERR_UNSUPPORTED, "the efficient heat-bath proposal is a 'chem' proposal");
  if (c->dev.cs.on) return fail(SQMC_ERR_BAD_ARG, "the context already proposes by Cauchy-Schwarz (sqmc_gpu_setup_cauchy_schwarz)");
  if (c->psit_shard) return fail(SQMC_ERR_UNSUPPORTED, "hf_to_psit with proposal_method fast_heatbath is not built");
  const int n = c->htab.norb, nc = c->htab.ncore;
  const long long n2 = (long long)n * n, n3 = n2 * n;
  HbHost *H = new HbHost();
  H->norb = n;
  H->size_same = (hbs_c2i(n, n) - 1) * n2 + (long long)(n - 1) * n + n;       // same_index(norb,norb,norb,norb), chemistry.f90:9154-9171
  H->size_opp = n3 * n;                                                       // opposite_index(norb,...), 9174-9192
  H->one.assign(n, 0.0); H->two.assign((size_t)4 * n2, 0.0);
  H->three_same.assign(n3, 0.0); H->three_opp.assign(n3, 0.0); H->q3_same.assign(n3, 0.0); H->q3_opp.assign(n3, 0.0);
  H->j3_same.assign(n3, 0); H->j3_opp.assign(n3, 0);
  H->four_same.assign(H->size_same, 0.f); H->four_opp.assign(H->size_opp, 0.f); H->q4_same.assign(H->size_same, 0.f); H->q4_opp.assign(H->size_opp, 0.f);
  H->j4_same.assign(H->size_same, 0); H->j4_opp.assign(H->size_opp, 0);
  const long long npairs = hbs_c2i(n, n);
  H->htot_same.assign((size_t)npairs * n, 0.0); H->htot_opp.assign(n3, 0.0);
  // 1-based accessors in the reference's column-major order
  auto ONE = [&](int i) -> double & { return H->one[i - 1]; };
  auto TWO = [&](int i, int j) -> double & { return H->two[(size_t)(i - 1) + (size_t)2 * n * (j - 1)]; };
  auto IX3 = [&](int i, int j, int k) -> size_t { return (size_t)(i - 1) + (size_t)n * (j - 1) + (size_t)n2 * (k - 1); };
  auto SAME = [&](int i, int j, int k, int l) -> size_t { return (size_t)((hbs_c2i(i, j) - 1) * n2 + (long long)(k - 1) * n + l - 1); };
  auto OPP = [&](int i, int j, int k, int l) -> size_t { return (size_t)((long long)(i - 1) * n3 + (long long)(j - 1) * n2 + (long long)(k - 1) * n + l - 1); };
  // ---- |H_ijkl| from the device, one first index at a time: same spin (i,j -> k,l up), opposite spin (i up, j dn -> k up, l dn) and its
  //      exchange partner (i up, j dn -> l up, k dn)
  std::vector<uint64_t> iu(n3), id(n3), ju(n3), jd(n3);
  std::vector<double> hs(n3), ho(n3), hx(n3);
  std::vector<double> all_o((size_t)(n + 1) * n3, -1.0), all_x((size_t)(n + 1) * n3, -1.0);      // |H| of the opposite-spin terms of every first index (-1: not visited)
  auto at = [&](int j, int k, int l) -> size_t { return ((size_t)(j - 1) * n + (k - 1)) * n + (l - 1); };
  for (int i = nc + 1; i <= n; i++) {
    for (int pass = 0; pass < 3; pass++) {
      for (int j = 1; j <= n; j++) for (int k = 1; k <= n; k++) for (int l = 1; l <= n; l++) {
        const size_t a = at(j, k, l);
        const uint64_t bi = 1ull << (i - 1), bj = 1ull << (j - 1), bk = 1ull << (k - 1), bl = 1ull << (l - 1);
        bool ok;
        if (pass == 0) { ok = !(i == j || k == l || i == k || i == l || j == k || j == l); iu[a] = bi | bj; id[a] = 0; ju[a] = bk | bl; jd[a] = 0; }
        else if (pass == 1) { ok = !(i == k || j == l); iu[a] = bi; id[a] = bj; ju[a] = bk; jd[a] = bl; }
        else { ok = !(i == l || j == k); iu[a] = bi; id[a] = bj; ju[a] = bl; jd[a] = bk; }
        if (!ok || j <= nc || k <= nc || l <= nc) { iu[a] = bi; id[a] = bi; ju[a] = bi; jd[a] = bi; }      // not visited by the loops: any pair (the value is not used)
      }
      int r = sqmc_gpu_hamiltonian_chem_batch(c, n3, iu.data(), id.data(), ju.data(), jd.data(), pass == 0 ? hs.data() : pass == 1 ? ho.data() : hx.data());
      if (r) { delete H; return r; }
    }
    // chemistry.f90:1061-1080 (same spin) in the loop order j, k, l
    for (int j = nc + 1; j <= n; j++) for (int k = nc + 1; k <= n; k++) for (int l = nc + 1; l <= n; l++) {
      if (!(i == k || j == l)) all_o[(size_t)i * n3 + at(j, k, l)] = fabs(ho[at(j, k, l)]);
      if (!(i == l || j == k)) all_x[(size_t)i * n3 + at(j, k, l)] = fabs(hx[at(j, k, l)]);
      if (i == j || k == l || i == k || i == l || j == k || j == l) continue;
      const double a = fabs(hs[at(j, k, l)]);
      ONE(i) = ONE(i) + a;
      TWO(i, j) = TWO(i, j) + a;
      TWO(n + i, n + j) = TWO(n + i, n + j) + a;
      H->three_same[IX3(i, j, k)] = H->three_same[IX3(i, j, k)] + a;
      float &f = H->four_same[SAME(i, j, k, l)];
      f = (float)((double)f + a);
    }
  }
  // chemistry.f90:1083-1110 (opposite spin): a second loop nest over all four indices, behind ALL same-spin terms
  for (int i = nc + 1; i <= n; i++) for (int j = nc + 1; j <= n; j++) for (int k = nc + 1; k <= n; k++) for (int l = nc + 1; l <= n; l++) {
    const double a = all_o[(size_t)i * n3 + at(j, k, l)], b = all_x[(size_t)i * n3 + at(j, k, l)];
    if (a >= 0.0) {            // i, k same spin; j, l same spin
      ONE(i) = ONE(i) + a;
      TWO(i, n + j) = TWO(i, n + j) + a;
      TWO(n + i, j) = TWO(n + i, j) + a;
      H->three_opp[IX3(i, j, k)] = H->three_opp[IX3(i, j, k)] + a;
      float &f = H->four_opp[OPP(i, j, k, l)];
      f = (float)((double)f + a);
    }
    if (b >= 0.0) {            // i, l same spin; j, k same spin
      ONE(i) = ONE(i) + b;
      TWO(i, n + j) = TWO(i, n + j) + b;
      TWO(n + i, j) = TWO(n + i, j) + b;
    }
  }
  all_o.clear(); all_o.shrink_to_fit(); all_x.clear(); all_x.shrink_to_fit();
  // ---- 1116-1149: Htot from the un-normalised four-index sums, the three-index tables normalised over their last index
  for (int i = nc + 1; i <= n; i++) for (int j = nc + 1; j <= n; j++) {
    double cs = 0.0, co = 0.0;
    for (int k = nc + 1; k <= n; k++) {
      for (int l = nc + 1; l <= n; l++) {
        if (i > j) H->htot_same[(size_t)(hbs_c2i(i, j) - 1) + (size_t)npairs * (k - 1)] = H->htot_same[(size_t)(hbs_c2i(i, j) - 1) + (size_t)npairs * (k - 1)] + (double)H->four_same[SAME(i, j, k, l)] * 2.0;
        H->htot_opp[IX3(i, j, k)] = H->htot_opp[IX3(i, j, k)] + (double)H->four_opp[OPP(i, j, k, l)] * 2.0;
      }
      cs = (k == nc + 1) ? H->three_same[IX3(i, j, k)] : H->three_same[IX3(i, j, k)] + cs;
      co = (k == nc + 1) ? H->three_opp[IX3(i, j, k)] : H->three_opp[IX3(i, j, k)] + co;
    }
    if (cs > 0.0) for (int k = 1; k <= n; k++) H->three_same[IX3(i, j, k)] = H->three_same[IX3(i, j, k)] / cs;
    if (co > 0.0) for (int k = 1; k <= n; k++) H->three_opp[IX3(i, j, k)] = H->three_opp[IX3(i, j, k)] / co;
  }
  // ---- 1151-1156: alias tables of the first hole
  std::vector<int> sm(2 * n + 2), lg(2 * n + 2), Jt(n);
  std::vector<double> pd(n), qd(n);
  for (int i = nc + 1; i <= n; i++) for (int j = nc + 1; j <= n; j++) for (int spin = 0; spin < 2; spin++) {
    std::vector<double> &P = spin ? H->three_opp : H->three_same, &Q = spin ? H->q3_opp : H->q3_same; std::vector<int32_t> &J = spin ? H->j3_opp : H->j3_same;
    for (int k = 1; k <= n; k++) pd[k - 1] = P[IX3(i, j, k)];
    hbs_alias<double>(n, pd.data(), sm.data(), lg.data(), Jt.data(), qd.data());
    for (int k = 1; k <= n; k++) { J[IX3(i, j, k)] = Jt[k - 1]; Q[IX3(i, j, k)] = qd[k - 1]; }
  }
  // ---- 1160-1190: the four-index tables normalised over their last index (a slice of norb consecutive entries), then their alias tables
  for (int i = nc + 1; i <= n; i++) for (int j = nc + 1; j <= n; j++) for (int k = nc + 1; k <= n; k++) {
    double cf = 0.0;                 // c_four_orbital_probabilities_* are real(rk) (chemistry.f90:63, 69): the slice is summed and divided in double, stored back as real
    for (int l = nc + 1; l <= n; l++) cf = (l == nc + 1) ? (double)H->four_same[SAME(i, j, k, l)] : cf + (double)H->four_same[SAME(i, j, k, l)];
    if (cf > 0.0) {
      float *p = &H->four_same[SAME(i, j, k, 1)];
      for (int l = 0; l < n; l++) p[l] = (float)((double)p[l] / cf);
      hbs_alias<float>(n, p, sm.data(), lg.data(), (int *)&H->j4_same[SAME(i, j, k, 1)], &H->q4_same[SAME(i, j, k, 1)]);
    }
    cf = 0.0;
    for (int l = nc + 1; l <= n; l++) cf = (l == nc + 1) ? (double)H->four_opp[OPP(i, j, k, l)] : cf + (double)H->four_opp[OPP(i, j, k, l)];
    if (cf > 0.0) {
      float *p = &H->four_opp[OPP(i, j, k, 1)];
      for (int l = 0; l < n; l++) p[l] = (float)((double)p[l] / cf);
      hbs_alias<float>(n, p, sm.data(), lg.data(), (int *)&H->j4_opp[OPP(i, j, k, 1)], &H->q4_opp[OPP(i, j, k, 1)]);
    }
  }
  // ---- check_heatbath_unbiased, 9330-9375: an orbital no other orbital is connected to by a one-body element has "unique symmetry"
  {
    const long long m = (long long)n * n;
    std::vector<uint64_t> a(m), z(m, 0), b(m); std::vector<double> h1(m);
    for (int p = 1; p <= n; p++) for (int q = 1; q <= n; q++) { a[(size_t)(p - 1) * n + q - 1] = 1ull << (p - 1); b[(size_t)(p - 1) * n + q - 1] = 1ull << (q - 1); }
    int r = sqmc_gpu_hamiltonian_chem_batch(c, m, a.data(), z.data(), b.data(), z.data(), h1.data());
    if (r) { delete H; return r; }
    int uniq = 0;
    for (int p = 1; p <= n; p++) {
      int s = 0;
      for (int q = 1; q <= n; q++) { if (p == q) continue; if (fabs(h1[(size_t)(p - 1) * n + q - 1]) > 1e-10) { s = 1; break; } }
      if (!s) uniq++;
    }
    H->n_orb_uniq_sym = uniq;
    H->unbiased = (std::max(c->htab.nup, c->htab.ndn) > uniq) ? 1 : 0;
  }
  if (is_heatbath_unbiased) *is_heatbath_unbiased = H->unbiased;
  sqmc_heatbath_tables t; memset(&t, 0, sizeof(t));
  t.norb = n; t.one_orbital_probabilities = H->one.data(); t.two_orbital_probabilities = H->two.data();
  t.three_orbital_probabilities_same_spin = H->three_same.data(); t.three_orbital_probabilities_opposite_spin = H->three_opp.data();
  t.J_three_orbital_probabilities_same_spin = H->j3_same.data(); t.J_three_orbital_probabilities_opposite_spin = H->j3_opp.data();
  t.q_three_orbital_probabilities_same_spin = H->q3_same.data(); t.q_three_orbital_probabilities_opposite_spin = H->q3_opp.data();
  t.size_same = H->size_same; t.size_opposite = H->size_opp;
  t.four_orbital_probabilities_same_spin = H->four_same.data(); t.four_orbital_probabilities_opposite_spin = H->four_opp.data();
  t.J_four_orbital_probabilities_same_spin = H->j4_same.data(); t.J_four_orbital_probabilities_opposite_spin = H->j4_opp.data();
  t.q_four_orbital_probabilities_same_spin = H->q4_same.data(); t.q_four_orbital_probabilities_opposite_spin = H->q4_opp.data();
  t.Htot_same = H->htot_same.data(); t.Htot_opposite = H->htot_opp.data();
  delete c->hb_host; c->hb_host = H;
  if (!H->unbiased) return SQMC_OK;          // the reference stops here ("Heatbath may be biased for this system!", 1219): the tables are kept for inspection, not installed
  return sqmc_gpu_set_heatbath_tables(c, &t);
}

int sqmc_gpu_get_heatbath_tables(sqmc_gpu_ctx *c, sqmc_heatbath_tables *t, int32_t *n_orb_uniq_sym) {
  if (!c || !t) return fail(SQMC_ERR_BAD_ARG, "null argument");
  if (!c->hb_host) return fail(SQMC_ERR_BAD_ARG, "sqmc_gpu_setup_efficient_heatbath has not been called");
  HbHost *H = c->hb_host;
  memset(t, 0, sizeof(*t));
  t->norb = H->norb; t->one_orbital_probabilities = H->one.data(); t->two_orbital_probabilities = H->two.data();
  t->three_orbital_probabilities_same_spin = H->three_same.data(); t->three_orbital_probabilities_opposite_spin = H->three_opp.data();
  t->J_three_orbital_probabilities_same_spin = H->j3_same.data(); t->J_three_orbital_probabilities_opposite_spin = H->j3_opp.data();
  t->q_three_orbital_probabilities_same_spin = H->q3_same.data(); t->q_three_orbital_probabilities_opposite_spin = H->q3_opp.data();
  t->size_same = H->size_same; t->size_opposite = H->size_opp;
  t->four_orbital_probabilities_same_spin = H->four_same.data(); t->four_orbital_probabilities_opposite_spin = H->four_opp.data();
  t->J_four_orbital_probabilities_same_spin = H->j4_same.data(); t->J_four_orbital_probabilities_opposite_spin = H->j4_opp.data();
  t->q_four_orbital_probabilities_same_spin = H->q4_same.data(); t->q_four_orbital_probabilities_opposite_spin = H->q4_opp.data();
  t->Htot_same = H->htot_same.data(); t->Htot_opposite = H->htot_opp.data();
  if (n_orb_uniq_sym) *n_orb_uniq_sym = H->n_orb_uniq_sym;
  return SQMC_OK;
}
static void hb_host_release(sqmc_gpu_ctx *c) { delete c->hb_host; c->hb_host = nullptr; }
