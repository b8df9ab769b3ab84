// Stand-alone driver of sqmc_amd/csrc/host_sort.h for tests/test_extrap_host_sort.py, built under the address and undefined-behaviour
// sanitizers.  Reads cases from the file named on the command line -- "n" and then n values, as hexadecimal floats --, sorts each in
// heap arrays of exactly n elements (so that a step outside them is seen), and prints per case one line with n, one with the sorted
// values and one with iorder (0-based, as it went in).
#include <stdio.h>
#include <stdlib.h>
#include "../sqmc_amd/csrc/host_sort.h"

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: extrap_sort_check <cases>\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  long long n;
  int cases = 0;
  while (fscanf(f, "%lld", &n) == 1) {
    double *a = (double *)malloc(n > 0 ? n * sizeof(double) : 1);
    int32_t *o = (int32_t *)malloc(n > 0 ? n * sizeof(int32_t) : 1);
    if (!a || !o) return 3;
    for (long long k = 0; k < n; k++) { if (fscanf(f, "%la", &a[k]) != 1) { fprintf(stderr, "short case\n"); return 2; } o[k] = (int32_t)k; }
    host_shell_sort_magnitude(n, a, o);
    printf("%lld\n", n);
    for (long long k = 0; k < n; k++) printf("%a ", a[k]);
    printf("\n");
    for (long long k = 0; k < n; k++) printf("%d ", (int)o[k]);
    printf("\n");
    free(a); free(o);
    cases++;
  }
  fclose(f);
  printf("all ok %d\n", cases);
  return 0;
}
