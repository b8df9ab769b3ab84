// host_sort.h -- the reference's order by magnitude, on the host.  No HIP in it: sqmc_gpu.hip includes it textually, and
// tests/extrap_sort_check.cpp compiles it alone.
#pragma once
#include <stdint.h>
#include <math.h>

// shell_sort_real_rank1_int_rank1 without consider_sign (generic_sort.f90:685-735): a(n) sorted by magnitude, greatest first, and
// iorder(n) carried along, by a shell sort with the gaps n/2, then gap * 5 / 11 (2 -> 1); an element moves past its neighbour
// only where that neighbour's magnitude is smaller, never where it is equal.  The sort is not stable, so for equal magnitudes
// only these statements give the reference's order.  Afterwards the whole of a changes sign if a[0] < 0.  Nothing is read for n <= 0.
static inline void host_shell_sort_magnitude(int64_t n, double *a, int32_t *iorder) {
  for (int64_t inc = n / 2; inc > 0; inc = inc == 2 ? 1 : inc * 5 / 11) {
    for (int64_t i = inc; i < n; i++) {
      const double t = a[i]; const int32_t ti = iorder[i];
      int64_t j = i;
      for (; j >= inc; j -= inc) {
        if (fabs(a[j - inc]) >= fabs(t)) break;
        a[j] = a[j - inc]; iorder[j] = iorder[j - inc];
      }
      a[j] = t; iorder[j] = ti;
    }
  }
  if (n > 0 && a[0] < 0) for (int64_t i = 0; i < n; i++) a[i] = -a[i];
}
