// orbhess_host_check.cpp -- the host arithmetic of the one-index transformation (sqmc_amd/csrc/orbopt_plan.h: orbhess_plan) and of the
// Fock plan it runs beside, checked for every orbital count the library accepts.  A stand-alone program: tests/test_orbhess_host.py
// builds it with the host compiler under the address and undefined-behaviour sanitizers and runs it as a child.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../sqmc_amd/csrc/orbopt_plan.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d, norb %d)\n", #c, __LINE__, n); return 1; } } while (0)

int main() {
  const int MAXORB = 64;
  int n = 0;
  // the shape at every size
  for (n = 1; n <= MAXORB; n++) {
    const OrbHessPlan p = orbhess_plan(n);
    CHECK(p.tm == (n > ORB_TM_SMALL_MAX ? 4 : 2) && p.tm == orbopt_plan(n).tm);
    CHECK(16 * p.tm >= n);                                 // the 16 x 16 owners of tm x tm register tiles cover norb x norb
    CHECK(p.npair == (long long)n * (n + 1) / 2);
    CHECK(p.ntile * ORB_SYM_TILE >= p.npair && (p.ntile - 1) * ORB_SYM_TILE < p.npair);
    CHECK(p.nsym == p.ntile * (p.ntile + 1) / 2);
    CHECK(ORB_T % ORB_SYM_TILE == 0 && ORB_SYM_TILE % (ORB_T / ORB_SYM_TILE) == 0);      // whole rows per pass of the symmetrising block
    CHECK((long long)2 * n * n * 8 <= 64 * 1024);          // the half pass's dynamic LDS needs no raised limit
    CHECK(p.npair * p.npair < (1ll << 31));                // the work buffer's largest index still fits the int of a block index times npair
  }
  printf("ok shapes of every size\n");
  // every (ti, tj) the symmetrising kernel decodes from its block index, and every pair it owns: each RS <= PQ exactly once
  for (n = 1; n <= MAXORB; n++) {
    const OrbHessPlan p = orbhess_plan(n);
    std::vector<unsigned char> seen((size_t)p.npair * p.npair, 0);
    for (long long b = 0; b < p.nsym; b++) {
      int ti = 0;
      while ((long long)(ti + 1) * (ti + 2) / 2 <= b) ti++;
      const int tj = (int)(b - (long long)ti * (ti + 1) / 2);
      CHECK(ti < p.ntile && tj >= 0 && tj <= ti);
      for (int y = 0; y < ORB_SYM_TILE; y++)
        for (int x = 0; x < ORB_SYM_TILE; x++) {
          const long long PQ = (long long)ti * ORB_SYM_TILE + y, RS = (long long)tj * ORB_SYM_TILE + x;
          if (PQ >= p.npair || RS > PQ) continue;
          CHECK(!seen[(size_t)PQ * p.npair + RS]);
          seen[(size_t)PQ * p.npair + RS] = 1;
        }
    }
    for (long long PQ = 0; PQ < p.npair; PQ++)
      for (long long RS = 0; RS <= PQ; RS++) CHECK(seen[(size_t)PQ * p.npair + RS]);
  }
  printf("ok one owner per packed entry\n");
  // the half pass's own pair numbering is one-to-one onto [0, npair), and the packed index of the largest pair fits an int
  for (n = 1; n <= MAXORB; n++) {
    const OrbHessPlan p = orbhess_plan(n);
    std::vector<unsigned char> seen((size_t)p.npair, 0);
    for (int P = 0; P < n; P++)
      for (int Q = 0; Q <= P; Q++) {
        const long long k = (long long)P * (P + 1) / 2 + Q;
        CHECK(k >= 0 && k < p.npair && !seen[(size_t)k]);
        seen[(size_t)k] = 1;
      }
    const long long A = p.npair + 1;                       // combine_2(norb + 1, norb + 1) of a dense pair order
    CHECK(A * (A - 1) / 2 + A < (1ll << 31));
  }
  printf("ok pair numbering\n");
  printf("all ok\n");
  return 0;
}
