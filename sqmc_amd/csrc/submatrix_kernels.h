// submatrix_kernels.h -- principal submatrix of a resident full-CSR matvec plan (sqmc_gpu_spmv_plan_submatrix)
// Textually included by sqmc_gpu.hip behind spmv_kernels.h (one translation unit); not a standalone header.
//
// dst(i, j) = src(sel[i], sel[j]), sel strictly ascending.  Every selected row is walked by one wavefront, 64 entries per round, twice:
// once to count the entries whose column is selected, once (behind the scan of the counts) to write them.  An entry's place in its
// row is the number of kept entries in front of it in the source row -- earlier rounds plus the lanes below in the ballot --, so a
// row's kept entries stay in the source order: no atomics, no LDS, and the result is entry for entry the plan that the builders make
// from the subset itself (spmv_kernels.h: diagonal first, stored columns ascending, then the transposed entries in increasing row).

// inv[r] = new index of source row r; the caller has set every word to -1.  flag[0] becomes nonzero if sel (1-based) leaves
// [1, n] or is not strictly ascending; a word of inv is written only for a row number in range.
__global__ void __launch_bounds__(TPB) k_sub_mark(const long long *__restrict__ sel, long long m, long long n, int *__restrict__ inv, u64 *__restrict__ flag) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const long long r = sel[i];
  const bool in_range = r >= 1 && r <= n;
  if (!in_range || (i > 0 && sel[i - 1] >= r)) flag[0] = 1;      // every writer stores the same word
  if (in_range) inv[r - 1] = (int)i;
}

// cnt[i] = entries of source row sel[i] whose column is selected.  One wavefront per selected row, laid out as k_spmv_wave.
// A refused sel (flag) is never dereferenced: the counts are zero and the door returns before the fill.
__global__ void __launch_bounds__(64 * SPMV_ROWS_PER_BLOCK) k_sub_count(const int *__restrict__ ptr, const int *__restrict__ col, const long long *__restrict__ sel,
                                                                        const int *__restrict__ inv, const u64 *__restrict__ flag, u64 *__restrict__ cnt, long long m) {
  const long long row = (long long)blockIdx.x * SPMV_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;                                            // wave-uniform: the ballots below see whole wavefronts
  if (flag[0]) { if (lane == 0) cnt[row] = 0; return; }
  const long long r = sel[row] - 1;
  const long long b = ptr[r], e = ptr[r + 1];
  u64 kept = 0;
  for (long long k0 = b; k0 < e; k0 += 64) {
    const long long k = k0 + lane;
    const bool keep = k < e && inv[col[k]] >= 0;
    kept += (u64)__popcll(__ballot(keep));
  }
  if (lane == 0) cnt[row] = kept;
}

// The same walk, writing: dptr[i] = off[i] (the exclusive scan of cnt), dptr[m] = nnz, and every kept entry at
// off[i] + entries kept in earlier rounds + kept lanes below this one, its column renumbered through inv.
__global__ void __launch_bounds__(64 * SPMV_ROWS_PER_BLOCK) k_sub_fill(const int *__restrict__ ptr, const int *__restrict__ col, const double *__restrict__ val,
                                                                       const long long *__restrict__ sel, const int *__restrict__ inv, const u64 *__restrict__ off,
                                                                       int *__restrict__ dptr, int *__restrict__ dcol, double *__restrict__ dval, long long m, long long nnz) {
  const long long row = (long long)blockIdx.x * SPMV_ROWS_PER_BLOCK + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  const long long r = sel[row] - 1;
  const long long b = ptr[r], e = ptr[r + 1];
  long long o = (long long)off[row];
  if (lane == 0) { dptr[row] = (int)o; if (row == m - 1) dptr[m] = (int)nnz; }
  const u64 below = (1ull << lane) - 1ull;
  for (long long k0 = b; k0 < e; k0 += 64) {
    const long long k = k0 + lane;
    const int c = k < e ? inv[col[k]] : -1;
    const u64 bal = __ballot(c >= 0);
    if (c >= 0) { const long long d = o + __popcll(bal & below); dcol[d] = c; dval[d] = val[k]; }
    o += __popcll(bal);
  }
}
