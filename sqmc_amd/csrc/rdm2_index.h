// rdm2_index.h -- the two index functions the Gram and expand kernels of the 2-RDM (rdm2_kernels.h, in rdm2_device.hip) and of the
// transition matrices (tdm_kernels.h, in tdm_device.hip) share: the entry of the Gram matrix a flat index names, and the flat index
// of a dense norb^4 block.  Device code only; textually included by both headers.
#pragma once
// flat index e = j (j + 1) / 2 + i, i <= j
__device__ __forceinline__ void rdm2_entry(long long e, long long *i, long long *j) {
  long long q = (long long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while (q > 0 && q * (q + 1) / 2 > e) q--;
  while ((q + 1) * (q + 2) / 2 <= e) q++;
  *j = q; *i = e - q * (q + 1) / 2;
}
// out[p + norb (q + norb (r + norb s))] = g
__device__ __forceinline__ void rdm2_put(double *__restrict__ out, int norb, int p, int q, int r, int s, double g) {
  out[(size_t)p + (size_t)norb * ((size_t)q + (size_t)norb * ((size_t)r + (size_t)norb * (size_t)s))] = g;
}
