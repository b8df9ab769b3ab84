// rdm2_launch.h -- the launches of the 2-RDM kernels, as plain functions.  The kernels (rdm2_kernels.h) are compiled in a translation
// unit of their own, rdm2_device.hip, so that they live in a code object of their own and the code object of sqmc_gpu.hip -- the
// walk's -- is the one it is without them.  The door (abi_rdm2.inc, in sqmc_gpu.hip) calls these; u64 / u32 and Rdm2Shape
// (rdm2_plan.h) are defined in front in both units.  Each enqueues on st and returns; errors surface in the door's hipGetLastError.
#pragma once
void rdm2_launch_emit(hipStream_t st, const u64 *binom, const u64 *su, const u64 *sd, const double *sc, long long n, const Rdm2Shape &sh,
                      u64 *sortkey, u32 *idx, u64 *K, u32 *P, double *V);
void rdm2_launch_pairkeys(hipStream_t st, const u32 *perm, const u32 *P, long long nrec, u64 *key2);
void rdm2_launch_sorted(hipStream_t st, const u32 *perm, const u64 *K, const u32 *P, const double *V, long long nrec, u64 *sK, u32 *sP, double *sV);
void rdm2_launch_colstart(hipStream_t st, const u32 *sP, long long nrec, int npairs, u32 *start);
// entries [0, eh) by a block each, [eh, nent) by a wavefront each
void rdm2_launch_gram(hipStream_t st, const u64 *sK, const double *sV, const u32 *start, const u32 *col, long long eh, long long nent, double *gram);
void rdm2_launch_expand(hipStream_t st, const double *gram, const u32 *col, long long nent, int kind, int norb, double *out);
