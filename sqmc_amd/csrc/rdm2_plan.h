// rdm2_plan.h -- the host arithmetic of a 2-RDM call: records per determinant, orbital pairs, the width of the intermediate key of a
// block, and the order in which the Gram kernel visits the columns.  Plain C++ (no HIP), so that tests/rdm2_host_check.cpp can run
// it under the host sanitizers.  Textually included by sqmc_gpu.hip.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#define RDM2_AA 0
#define RDM2_BB 1
#define RDM2_AB 2
#define RDM2_HEAVY 512u         // a column at least this long: its entries with longer columns get a whole block each

struct Rdm2Shape {
  int kind, norb, nup, ndn;
  int R;                         // records of one determinant: C(nup, 2), C(ndn, 2), nup ndn
  int npairs;                    // columns: norb (norb - 1) / 2 pairs r < s, or norb^2 pairs (r, s)
  int kbits, pbits;              // bits of the key of K (0 .. 64) and of the pair index (>= 1)
  int oneword;                   // pair and K share one 64-bit sort word
  int fits;                      // the key space of K fits 64 bits
  unsigned long long n_dn_k;     // C(norb, dn electrons of K): the stride of the up rank in the key
};

// C(n, k) in 128 bits, saturating at 2^127 (n <= 64 here, so nothing saturates; the guard keeps the arithmetic defined)
static inline unsigned __int128 rdm2_choose(int n, int k) {
  if (k < 0 || k > n) return 0;
  unsigned __int128 r = 1;
  for (int q = 1; q <= k; q++) {
    if (r > (((unsigned __int128)1) << 120)) return ((unsigned __int128)1) << 127;
    r = r * (unsigned)(n - k + q) / (unsigned)q;      // exact: r holds C(n - k + q - 1, q - 1), and q divides r (n - k + q)
  }
  return r;
}
static inline int rdm2_bits_for(unsigned __int128 count) {      // the fewest bits that hold every value below count
  int b = 0;
  while (b < 128 && ((((unsigned __int128)1) << b) < count)) b++;
  return b;
}
static inline Rdm2Shape rdm2_shape(int kind, int norb, int nup, int ndn) {
  Rdm2Shape s{};
  s.kind = kind; s.norb = norb; s.nup = nup; s.ndn = ndn;
  const int ku = kind == RDM2_AA ? nup - 2 : kind == RDM2_AB ? nup - 1 : nup, kd = kind == RDM2_BB ? ndn - 2 : kind == RDM2_AB ? ndn - 1 : ndn;
  s.R = kind == RDM2_AA ? nup * (nup - 1) / 2 : kind == RDM2_BB ? ndn * (ndn - 1) / 2 : nup * ndn;
  if (ku < 0 || kd < 0) s.R = 0;
  s.npairs = kind == RDM2_AB ? norb * norb : norb * (norb - 1) / 2;
  s.fits = 1;
  if (s.R == 0 || s.npairs == 0) { s.R = 0; s.pbits = 1; return s; }
  const unsigned __int128 nu = rdm2_choose(norb, ku), nd = rdm2_choose(norb, kd);
  const unsigned __int128 space = nu * nd;      // both below 2^63: the product fits 128 bits
  s.n_dn_k = (unsigned long long)nd;
  s.fits = space <= (((unsigned __int128)1) << 64);
  s.kbits = s.fits ? rdm2_bits_for(space) : 128;
  s.pbits = rdm2_bits_for((unsigned __int128)s.npairs); if (s.pbits < 1) s.pbits = 1;
  s.oneword = s.fits && s.kbits + s.pbits <= 64;
  return s;
}

// The non-empty columns, longest first (ties: lower pair index first): col[k] = pair index of rank k.  start: npairs + 1 offsets
// of the columns in the sorted records.  *n_heavy = how many are at least RDM2_HEAVY long.  An entry of the Gram matrix is a pair
// of ranks i <= j, at flat index j (j + 1) / 2 + i: column j is the shorter one, so the flat order runs from the most work to the least.
static inline void rdm2_column_order(const std::vector<uint32_t> &start, std::vector<uint32_t> &col, long long *n_heavy) {
  col.clear(); *n_heavy = 0;
  if (start.size() < 2) return;
  const size_t np = start.size() - 1;
  for (size_t p = 0; p < np; p++) if (start[p + 1] > start[p]) col.push_back((uint32_t)p);
  std::stable_sort(col.begin(), col.end(), [&](uint32_t a, uint32_t b) { return start[a + 1] - start[a] > start[b + 1] - start[b]; });
  for (uint32_t p : col) if (start[p + 1] - start[p] >= RDM2_HEAVY) ++*n_heavy;
}
