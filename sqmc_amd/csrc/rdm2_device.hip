// rdm2_device.hip -- the second translation unit of libsqmc_gpu: the 2-RDM kernels and their launches (rdm2_launch.h), nothing else.
// Its kernels make a code object of their own; sqmc_gpu.hip holds the door and every other kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "chem_device.h"        // u64, ctz64, bit64, colex_rank and the layout of the binomial table
typedef unsigned int u32;
#ifndef TPB
#define TPB 256
#endif
#include "rdm2_plan.h"
#include "rdm2_kernels.h"
#include "rdm2_launch.h"

static inline unsigned rdm2_nblk(long long n) { return (unsigned)((n + TPB - 1) / TPB); }

void rdm2_launch_emit(hipStream_t st, const u64 *binom, const u64 *su, const u64 *sd, const double *sc, long long n, const Rdm2Shape &sh,
                      u64 *sortkey, u32 *idx, u64 *K, u32 *P, double *V) {
  hipLaunchKernelGGL(k_rdm2_emit, dim3(rdm2_nblk(n * sh.R)), dim3(TPB), 0, st, binom, su, sd, sc, n, sh, sortkey, idx, K, P, V);
}
void rdm2_launch_pairkeys(hipStream_t st, const u32 *perm, const u32 *P, long long nrec, u64 *key2) {
  hipLaunchKernelGGL(k_rdm2_pairkeys, dim3(rdm2_nblk(nrec)), dim3(TPB), 0, st, perm, P, nrec, key2);
}
void rdm2_launch_sorted(hipStream_t st, const u32 *perm, const u64 *K, const u32 *P, const double *V, long long nrec, u64 *sK, u32 *sP, double *sV) {
  hipLaunchKernelGGL(k_rdm2_sorted, dim3(rdm2_nblk(nrec)), dim3(TPB), 0, st, perm, K, P, V, nrec, sK, sP, sV);
}
void rdm2_launch_colstart(hipStream_t st, const u32 *sP, long long nrec, int npairs, u32 *start) {
  hipLaunchKernelGGL(k_rdm2_colstart, dim3(rdm2_nblk((long long)npairs + 1)), dim3(TPB), 0, st, sP, nrec, npairs, start);
}
void rdm2_launch_gram(hipStream_t st, const u64 *sK, const double *sV, const u32 *start, const u32 *col, long long eh, long long nent, double *gram) {
  if (eh > 0) hipLaunchKernelGGL(k_rdm2_gram<256>, dim3((unsigned)eh), dim3(256), 0, st, sK, sV, start, col, 0ll, eh, gram);
  if (nent > eh) hipLaunchKernelGGL(k_rdm2_gram<64>, dim3((unsigned)((nent - eh + 3) / 4)), dim3(256), 0, st, sK, sV, start, col, eh, nent, gram);
}
void rdm2_launch_expand(hipStream_t st, const double *gram, const u32 *col, long long nent, int kind, int norb, double *out) {
  hipLaunchKernelGGL(k_rdm2_expand, dim3(rdm2_nblk(nent)), dim3(TPB), 0, st, gram, col, nent, kind, norb, out);
}
