// spawn_prof.h -- the stamps of the instrumented build of k_spawn.  Textually included by sqmc_gpu.hip in front of bucket_partition.h
// (whose boundary blocks stamp their phases) and walk_kernels.h; not a standalone header.
#pragma once

// -DSPAWN_PROF (tools/spawn_prof.py): every block of k_spawn leaves wall-clock stamps, 8 words per block: [0] start, [1..4] phases,
// [5] end, [6] what the block was (PROF_KIND).  PROF_B stamps behind a barrier of the block (the spare blocks: when all of it is through).
#ifdef SPAWN_PROF
__device__ unsigned long long g_prof[8 * 8192];
#define PROF(K) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_prof[blockIdx.x * 8 + (K)] = wall_clock64(); } while (0)
#define PROF_B(K) do { __syncthreads(); PROF(K); } while (0)
#define PROF_KIND(V) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_prof[blockIdx.x * 8 + 6] = (V); } while (0)
extern "C" int sqmc_gpu_debug_prof(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(g_prof)); }
#else
#define PROF(K)
#define PROF_B(K)
#define PROF_KIND(V)
#endif
#define PROF_SPAWNING 0
#define PROF_FINAL_SUMS 1
#define PROF_HII_QUEUE 2
#define PROF_PRJ_ROWS 3
#define PROF_BOUNDARIES 4              // the block that finds today's positions (before the split: the one boundary block)
#define PROF_BOUNDARIES_NEXT 5         // the block that makes the next boundaries
