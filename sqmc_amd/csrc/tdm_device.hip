// tdm_device.hip -- the fourth translation unit of libsqmc_gpu: the transition-density-matrix kernels (tdm_kernels.h) and their
// launches (tdm_launch.h), nothing else.  Its kernels make a code object of their own; the code objects of sqmc_gpu.hip,
// rdm2_device.hip and orbopt_device.hip are the ones they are without them.  The records come from rdm2_device.hip's kernels through
// rdm2_launch.h, called by the door.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "chem_device.h"        // u64, ctz64, bit64, popc64, maskr64, det_key, ChemDev and the layout of the binomial table
typedef unsigned int u32;
#ifndef TPB
#define TPB 256
#endif
#include "rdm2_plan.h"
#include "tdm_launch.h"
#include "tdm_kernels.h"

static inline unsigned tdm_nblk(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

void tdm_launch_bra(hipStream_t st, const double *sc_bra, long long n, const Rdm2Shape &sh, double *U) {
  hipLaunchKernelGGL(k_tdm2_bra, dim3(tdm_nblk(n * sh.R)), dim3(TPB), 0, st, sc_bra, n, sh, U);
}
void tdm_launch_sorted(hipStream_t st, const u32 *perm, const u64 *K, const u32 *P, const double *U, const double *W, long long nrec,
                       u64 *sK, u32 *sP, double *sU, double *sW) {
  hipLaunchKernelGGL(k_tdm2_sorted, dim3(tdm_nblk(nrec)), dim3(TPB), 0, st, perm, K, P, U, W, nrec, sK, sP, sU, sW);
}
void tdm_launch_gram(hipStream_t st, const u64 *sK, const double *sU, const double *sW, const u32 *start, const u32 *col, long long eh, long long nent, double *gram) {
  if (eh > 0) hipLaunchKernelGGL(k_tdm2_gram<256>, dim3((unsigned)eh), dim3(256), 0, st, sK, sU, sW, start, col, 0ll, eh, gram);
  if (nent > eh) hipLaunchKernelGGL(k_tdm2_gram<64>, dim3((unsigned)((nent - eh + 3) / 4)), dim3(256), 0, st, sK, sU, sW, start, col, eh, nent, gram);
}
void tdm_launch_expand(hipStream_t st, const double *gram, const u32 *col, long long nent, int kind, int norb, double *out) {
  hipLaunchKernelGGL(k_tdm2_expand, dim3(tdm_nblk(nent)), dim3(TPB), 0, st, gram, col, nent, kind, norb, out);
}
void tdm_launch_one(hipStream_t st, const ChemDev &dev, const u64 *su, const u64 *sd, const double *s_bra, const double *s_ket, long long n, const u64 *skey,
                    int norb, const unsigned char *sym, double *partial, double *tdm) {
  const int nchunks = (int)((n + TDM1_CHUNK - 1) / TDM1_CHUNK);
  hipLaunchKernelGGL(k_tdm1_terms, dim3(nchunks, norb * (norb + 1) / 2, 2), dim3(TDM1_T), 0, st, dev, su, sd, s_bra, s_ket, n, skey, norb, sym, partial);
  hipLaunchKernelGGL(k_tdm1_sum, dim3(tdm_nblk((long long)norb * norb)), dim3(TPB), 0, st, (const double *)partial, nchunks, norb, tdm);
}
