// orbopt_device.hip -- the third translation unit of libsqmc_gpu: the orbital-gradient and Hessian-vector kernels and their launches
// (orbopt_launch.h), nothing else.  Its kernels make a code object of their own; sqmc_gpu.hip holds the door and every other kernel but the 2-RDM's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "orbopt_plan.h"
#include "orbopt_kernels.h"
#include "orbopt_launch.h"

static inline unsigned orbopt_nblk(int n) { return (unsigned)((n + ORB_T - 1) / ORB_T); }

void orbopt_launch_fock(hipStream_t st, const OrbPlan &plan, const double *ints, const int *pair, int hbase, const double *D, const double *G, int norb,
                        double *part, double *F) {
  const int nn = norb * norb;
  const size_t lds = (size_t)nn * sizeof(int);
  if (plan.tm == 4) hipLaunchKernelGGL(k_orb_fock_part<4>, dim3((unsigned)plan.nblocks), dim3(ORB_T), lds, st, ints, pair, G, norb, plan.K, plan.nchunks, plan.cpb, part);
  else hipLaunchKernelGGL(k_orb_fock_part<2>, dim3((unsigned)plan.nblocks), dim3(ORB_T), lds, st, ints, pair, G, norb, plan.K, plan.nchunks, plan.cpb, part);
  hipLaunchKernelGGL(k_orb_fock_reduce, dim3(orbopt_nblk(nn)), dim3(ORB_T), 0, st, ints, pair, hbase, D, part, norb, plan.nblocks, F);
}
void orbopt_launch_grad(hipStream_t st, const double *F, int norb, double *grad) {
  hipLaunchKernelGGL(k_orb_grad, dim3(orbopt_nblk(norb * norb)), dim3(ORB_T), 0, st, F, norb, grad);
}
void orbopt_launch_hdiag(hipStream_t st, const double *ints, const int *pair, int hbase, const double *D, const double *G, const double *F, int norb, double *hd) {
  hipLaunchKernelGGL(k_orb_hdiag, dim3((unsigned)(norb * norb)), dim3(ORB_HD_T), 0, st, ints, pair, hbase, D, G, F, norb, hd);
}
void orbopt_launch_oneidx_half(hipStream_t st, const OrbHessPlan &hp, const double *ints, const int *pair, const int *pidx, int hbase, const double *kap, int norb, double *work) {
  const size_t lds = (size_t)2 * norb * norb * sizeof(double);
  if (hp.tm == 4) hipLaunchKernelGGL((k_orb_oneidx_half<4, false>), dim3((unsigned)hp.npair), dim3(ORB_T), lds, st, ints, pair, pidx, hbase, kap, norb, work);
  else hipLaunchKernelGGL((k_orb_oneidx_half<2, false>), dim3((unsigned)hp.npair), dim3(ORB_T), lds, st, ints, pair, pidx, hbase, kap, norb, work);
}
void orbopt_launch_oneidx_sym(hipStream_t st, const OrbHessPlan &hp, const double *ints, const int *pair, const int *pidx, int hbase, const double *kap, int norb,
                              const double *work, double *out) {
  const size_t lds = (size_t)2 * norb * norb * sizeof(double);
  hipLaunchKernelGGL(k_orb_oneidx_sym, dim3((unsigned)hp.nsym), dim3(ORB_T), 0, st, work, pidx, (int)hp.npair, out);
  if (hp.tm == 4) hipLaunchKernelGGL((k_orb_oneidx_half<4, true>), dim3(1), dim3(ORB_T), lds, st, ints, pair, pidx, hbase, kap, norb, out);
  else hipLaunchKernelGGL((k_orb_oneidx_half<2, true>), dim3(1), dim3(ORB_T), lds, st, ints, pair, pidx, hbase, kap, norb, out);
}
void orbopt_launch_sigma(hipStream_t st, const double *Ft, const double *g, const double *kap, int norb, double *sigma) {
  hipLaunchKernelGGL(k_orb_sigma, dim3(orbopt_nblk(norb * norb)), dim3(ORB_T), 0, st, Ft, g, kap, norb, sigma);
}
