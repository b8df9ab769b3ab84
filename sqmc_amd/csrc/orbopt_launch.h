// orbopt_launch.h -- the launches of the orbital-gradient kernels, as plain functions.  The kernels (orbopt_kernels.h) are compiled in
// a translation unit of their own, orbopt_device.hip, so that the code object of sqmc_gpu.hip -- the walk's -- is the one it is
// without them.  The doors (abi_orbopt.inc and abi_orbhess.inc, in sqmc_gpu.hip) call these; OrbPlan (orbopt_plan.h) is defined in front in both units.
// Each enqueues on st and returns; errors surface in the door's hipGetLastError.
#pragma once
// part: plan.nblocks tiles of norb^2 doubles, every entry written
void orbopt_launch_fock(hipStream_t st, const OrbPlan &plan, const double *ints, const int *pair, int hbase, const double *D, const double *G, int norb,
                        double *part, double *F);
void orbopt_launch_grad(hipStream_t st, const double *F, int norb, double *grad);
void orbopt_launch_hdiag(hipStream_t st, const double *ints, const int *pair, int hbase, const double *D, const double *G, const double *F, int norb, double *hd);
// The one-index transformation of the packed table `ints` by kap (norb^2 doubles, kap[a norb + P]) into `out`, which the caller has
// zeroed: the half pass into work (npair^2 doubles, every entry written), the symmetrising pass, the one-body block.  pidx: the
// npair pair indices in the kernels' own numbering.  The dynamic LDS of the half pass is 2 norb^2 doubles (64 KB at 64 orbitals).
void orbopt_launch_oneidx_half(hipStream_t st, const OrbHessPlan &hp, const double *ints, const int *pair, const int *pidx, int hbase, const double *kap, int norb, double *work);
void orbopt_launch_oneidx_sym(hipStream_t st, const OrbHessPlan &hp, const double *ints, const int *pair, const int *pidx, int hbase, const double *kap, int norb,
                              const double *work, double *out);
// sigma = gradient formula on Ft + 1/2 [kap, g]
void orbopt_launch_sigma(hipStream_t st, const double *Ft, const double *g, const double *kap, int norb, double *sigma);
