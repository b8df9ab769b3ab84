// orbopt_plan.h -- the shape of the orbital-gradient kernels as plain host arithmetic: the register tile, the K chunk and the K split of
// the Fock GEMM (orbopt_kernels.h).  Included by both translation units (the door sizes its partial tiles from it, the launches their
// grids); names no HIP header.  sqmc_gpu_debug_orbopt_plan shows it to the tests.
#pragma once

#define ORB_T 256                // threads of a Fock block: 16 x 16 owners of TM x TM register tiles
#define ORB_KC 16                // (q, r, s) triples staged into LDS at a time
#define ORB_MAX_BLOCKS 512       // K is split over at most this many blocks (2 per compute unit of a 256-unit chip)
#define ORB_TM_SMALL_MAX 32      // up to here 2 x 2 register tiles cover the norb x norb tile, above 4 x 4 (up to 64)
#define ORB_HD_T 64              // threads (one wavefront) of the owner of one hdiag[p, q]
#define ORB_SYM_TILE 32          // k_orb_oneidx_sym adds the work buffer to its transpose in tiles of this many pairs a side

struct OrbPlan {
  int tm, nt;                    // register tile, and the 16 tm rows / columns a block covers (>= norb)
  long long K, nchunks, cpb, nblocks;      // norb^3 triples, in chunks of ORB_KC, cpb consecutive chunks per block, nblocks partial tiles
};
static inline OrbPlan orbopt_plan(int norb) {
  OrbPlan p;
  p.tm = norb > ORB_TM_SMALL_MAX ? 4 : 2; p.nt = 16 * p.tm;
  p.K = (long long)norb * norb * norb;
  p.nchunks = (p.K + ORB_KC - 1) / ORB_KC;
  p.cpb = (p.nchunks + ORB_MAX_BLOCKS - 1) / ORB_MAX_BLOCKS;
  if (p.cpb < 1) p.cpb = 1;
  p.nblocks = (p.nchunks + p.cpb - 1) / p.cpb;
  return p;
}

// The one-index transformation (k_orb_oneidx_half, k_orb_oneidx_sym): the register tile of the half pass (the Fock GEMM's switch), the
// norb (norb + 1) / 2 orbital pairs = blocks of the half pass = side of the work buffer, and the tiles of the symmetrising pass: one
// block per pair of tiles (ti >= tj).  sqmc_gpu_debug_orbhess_plan shows it to the tests.
struct OrbHessPlan { int tm; long long npair, ntile, nsym; };
static inline OrbHessPlan orbhess_plan(int norb) {
  OrbHessPlan p;
  p.tm = norb > ORB_TM_SMALL_MAX ? 4 : 2;
  p.npair = (long long)norb * (norb + 1) / 2;
  p.ntile = (p.npair + ORB_SYM_TILE - 1) / ORB_SYM_TILE;
  p.nsym = p.ntile * (p.ntile + 1) / 2;
  return p;
}
