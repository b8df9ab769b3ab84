// tdm_launch.h -- the launches of the transition-density-matrix kernels (tdm_kernels.h), as plain functions beside those of
// rdm2_launch.h: the kernels are compiled in a translation unit and code object of their own, tdm_device.hip, and the doors
// (abi_tdm.inc, in sqmc_gpu.hip) call these.  u64 / u32, ChemDev (chem_device.h) and Rdm2Shape (rdm2_plan.h) are defined in front in
// both units.  Each enqueues on st and returns; errors surface in the door's hipGetLastError.
#pragma once
#define TDM1_T 256               // threads of a one-body block: RDM_T
#define TDM1_CHUNK 1024          // determinants of a one-body block's chunk: RDM_CHUNK
void tdm_launch_bra(hipStream_t st, const double *sc_bra, long long n, const Rdm2Shape &sh, double *U);
void tdm_launch_sorted(hipStream_t st, const u32 *perm, const u64 *K, const u32 *P, const double *U, const double *W, long long nrec,
                       u64 *sK, u32 *sP, double *sU, double *sW);
// entries [0, eh) by a block each, [eh, nent) by a wavefront each; gram: 2 nent doubles
void tdm_launch_gram(hipStream_t st, const u64 *sK, const double *sU, const double *sW, const u32 *start, const u32 *col, long long eh, long long nent, double *gram);
void tdm_launch_expand(hipStream_t st, const double *gram, const u32 *col, long long nent, int kind, int norb, double *out);
// partial: nchunks * norb (norb + 1) * 2 doubles, nchunks = ceil(n / TDM1_CHUNK); tdm: norb^2 doubles, every entry written
void tdm_launch_one(hipStream_t st, const ChemDev &dev, const u64 *su, const u64 *sd, const double *s_bra, const double *s_ket, long long n, const u64 *skey,
                    int norb, const unsigned char *sym, double *partial, double *tdm);
