// The host arithmetic of a 2-RDM call (sqmc_amd/csrc/rdm2_plan.h) alone: a stand-alone program for the address and
// undefined-behaviour sanitizers of the host compiler.  Prints "ok <property>" per property and "all ok".
#include "../sqmc_amd/csrc/rdm2_plan.h"
#include <stdio.h>
#include <stdlib.h>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static unsigned __int128 slow_choose(int n, int k) {      // Pascal's rule
  if (k < 0 || k > n) return 0;
  static unsigned __int128 t[66][66]; static bool done = false;
  if (!done) { for (int a = 0; a < 66; a++) for (int b = 0; b <= a; b++) t[a][b] = (b == 0 || b == a) ? 1 : t[a - 1][b - 1] + t[a - 1][b]; done = true; }
  return t[n][k];
}

int main() {
  for (int n = 0; n <= 64; n++) for (int k = -1; k <= n + 1; k++) CHECK(rdm2_choose(n, k) == slow_choose(n, k));
  printf("ok binomials up to 64\n");
  CHECK(rdm2_bits_for(0) == 0 && rdm2_bits_for(1) == 0 && rdm2_bits_for(2) == 1 && rdm2_bits_for(3) == 2 && rdm2_bits_for(1024) == 10 && rdm2_bits_for(1025) == 11);
  CHECK(rdm2_bits_for(((unsigned __int128)1) << 64) == 64 && rdm2_bits_for((((unsigned __int128)1) << 64) + 1) == 65);
  printf("ok key widths\n");
  // every sector of every orbital count: records, pairs, and that pair and key fit the word whenever oneword says so
  for (int norb = 1; norb <= 64; norb++)
    for (int nup = 0; nup <= norb; nup++)
      for (int ndn = 0; ndn <= norb; ndn += (norb > 24 ? 5 : 1))
        for (int kind = 0; kind < 3; kind++) {
          const Rdm2Shape s = rdm2_shape(kind, norb, nup, ndn);
          const int want = kind == RDM2_AA ? nup * (nup - 1) / 2 : kind == RDM2_BB ? ndn * (ndn - 1) / 2 : nup * ndn;
          CHECK(s.R == ((kind != RDM2_AB && norb < 2) ? 0 : want));
          if (!s.R) { CHECK(s.fits); continue; }
          CHECK(s.npairs == (kind == RDM2_AB ? norb * norb : norb * (norb - 1) / 2));
          CHECK(s.pbits >= 1 && ((unsigned long long)s.npairs <= (1ull << s.pbits)));
          const int ku = kind == RDM2_AA ? nup - 2 : kind == RDM2_AB ? nup - 1 : nup, kd = kind == RDM2_BB ? ndn - 2 : kind == RDM2_AB ? ndn - 1 : ndn;
          const unsigned __int128 space = slow_choose(norb, ku) * slow_choose(norb, kd);
          CHECK(s.fits == (space <= (((unsigned __int128)1) << 64)));
          if (s.fits) { CHECK(s.n_dn_k == (unsigned long long)slow_choose(norb, kd)); CHECK(s.kbits <= 64 && (s.kbits == 64 || space <= (((unsigned __int128)1) << s.kbits))); }
          if (s.oneword) CHECK(s.fits && s.kbits + s.pbits <= 64 && s.kbits <= 63);
          if (s.fits && !s.oneword) CHECK(s.kbits + s.pbits > 64);
        }
  printf("ok shapes of every sector\n");
  { const Rdm2Shape a = rdm2_shape(RDM2_AB, 26, 4, 4); CHECK(a.oneword && a.R == 16 && a.npairs == 676 && a.pbits == 10 && a.kbits == 23); }
  { const Rdm2Shape a = rdm2_shape(RDM2_AB, 64, 32, 32); CHECK(!a.fits); const Rdm2Shape b = rdm2_shape(RDM2_AA, 64, 20, 20); CHECK(!b.fits || !b.oneword); }
  { const Rdm2Shape a = rdm2_shape(RDM2_AB, 64, 8, 7); CHECK(a.fits && !a.oneword && a.kbits == 56 && a.pbits == 12); }
  printf("ok one word, two passes, refused\n");
  // column order: longest first, ties by pair index, empties left out, heavy count
  srand(7);
  for (int rep = 0; rep < 200; rep++) {
    const int np = 1 + rand() % 300;
    std::vector<uint32_t> start(np + 1, 0), col;
    for (int p = 0; p < np; p++) { const int r = rand() % 4; start[p + 1] = start[p] + (r == 0 ? 0 : r == 1 ? rand() % 5 : r == 2 ? rand() % 700 : 400 + rand() % 3000); }
    long long heavy = -1;
    rdm2_column_order(start, col, &heavy);
    long long h = 0; size_t nonempty = 0;
    for (int p = 0; p < np; p++) { const uint32_t len = start[p + 1] - start[p]; if (len) nonempty++; if (len >= RDM2_HEAVY) h++; }
    CHECK(col.size() == nonempty && heavy == h);
    for (size_t k = 0; k + 1 < col.size(); k++) {
      const uint32_t a = start[col[k] + 1] - start[col[k]], b = start[col[k + 1] + 1] - start[col[k + 1]];
      CHECK(a > b || (a == b && col[k] < col[k + 1]));
    }
    for (size_t k = 0; k < col.size(); k++) CHECK(col[k] < (uint32_t)np && (k >= (size_t)heavy) == (start[col[k] + 1] - start[col[k]] < RDM2_HEAVY));
  }
  { std::vector<uint32_t> none, one(1, 0), col; long long heavy = 5; rdm2_column_order(none, col, &heavy); CHECK(col.empty() && heavy == 0); rdm2_column_order(one, col, &heavy); CHECK(col.empty()); }
  printf("ok column order\n");
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("all ok\n");
  return 0;
}
