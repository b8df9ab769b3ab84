// orbopt_launch.h -- the launches of the orbital-gradient kernels, as plain functions.  The kernels (orbopt_kernels.h) are compiled in
// a translation unit of their own, orbopt_device.hip, so that the code object of sqmc_gpu.hip -- the walk's -- is the one it is
// without them.  The door (abi_orbopt.inc, in sqmc_gpu.hip) calls these; OrbPlan (orbopt_plan.h) is defined in front in both units.
// Each enqueues on st and returns; errors surface in the door's hipGetLastError.
#pragma once
// part: plan.nblocks tiles of norb^2 doubles, every entry written
void orbopt_launch_fock(hipStream_t st, const OrbPlan &plan, const double *ints, const int *pair, int hbase, const double *D, const double *G, int norb,
                        double *part, double *F);
void orbopt_launch_grad(hipStream_t st, const double *F, int norb, double *grad);
void orbopt_launch_hdiag(hipStream_t st, const double *ints, const int *pair, int hbase, const double *D, const double *G, const double *F, int norb, double *hd);
