"""A plain reference for the linear-algebra side (sparse symmetric matvec, CSR builder, Davidson), independent of the library and
of the oracle: it imports neither.  Three parts.

Storage.  The project's format for a symmetric matrix: counts[n] entries per row, then per row the diagonal first and the
columns j < i after it, 1-based, in idx / val.  `storage` builds it from a {(i, j): a} dictionary, `dense` expands it.

Exact matvec.  Every product a_ij x_j is split into its rounded value and its rounding error (Dekker's two-product on Veltkamp
halves, exact while nothing over- or underflows), and math.fsum adds the 2 L_i pieces of a row without error, so exact[i] is the
true sum rounded once.  A double-precision sum of L products in ANY order, fused or not, commits at most L roundings on the way
of a term, hence |y_i - true_i| <= gamma_L sum_j |a_ij x_j| with gamma_m = m u / (1 - m u), u = 2^-53; the tests use
gamma_{L+1}: the extra u pays for the one rounding of the reference itself.

Eigenvalues.  LAPACK on the dense matrix (n <= 2000); for an arrow matrix the lowest root of its secular equation and for a
symmetric tridiagonal matrix Sturm-count bisection, both in long double, which need no dense matrix and reach n = 300 001."""
import math

import numpy as np

U = 2.0 ** -53
LADDER = (1, 2, 63, 64, 65, 127, 128, 129, 4097)


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------------------------------------------------------------- storage
def storage(n, entries):
    """entries: {(i, j): a}, 0-based, each unordered pair once (either orientation); a row without a diagonal gets a stored 0.0.
    Returns counts, idx (1-based, diagonal first, then j < i ascending), val."""
    rows = [[] for _ in range(n)]
    diag = [0.0] * n
    for (i, j), a in entries.items():
        if i == j:
            diag[i] = a
        else:
            assert (j, i) not in entries
            rows[max(i, j)].append((min(i, j), a))
    counts = np.zeros(n, np.int64); idx = []; val = []
    for i in range(n):
        rows[i].sort(key=lambda t: t[0])
        counts[i] = 1 + len(rows[i])
        idx.append(i + 1); val.append(diag[i])
        idx.extend(j + 1 for j, _ in rows[i]); val.extend(a for _, a in rows[i])
    return counts, np.array(idx, np.int64), np.array(val, np.float64)


def storage_from_dense(A):
    n = len(A)
    return storage(n, {(i, j): float(A[i, j]) for i in range(n) for j in range(i + 1) if i == j or A[i, j] != 0.0})


def triplets(counts, idx, val):
    """(row, col, value) of the FULL matrix: every stored entry, and its mirror image when it is off the diagonal"""
    counts = np.asarray(counts, np.int64); idx = np.asarray(idx, np.int64); val = np.asarray(val, np.float64)
    r = np.repeat(np.arange(len(counts)), counts); c = idx - 1
    off = r != c
    return np.concatenate((r, c[off])), np.concatenate((c, r[off])), np.concatenate((val, val[off]))


def dense(counts, idx, val):
    n = len(counts)
    r, c, v = triplets(counts, idx, val)
    A = np.zeros((n, n)); A[r, c] = v
    return A


def diagonal_of(counts, val):
    return np.asarray(val, np.float64)[np.concatenate(([0], np.cumsum(counts)))[:-1]]


def norm1(counts, idx, val):
    r, _, v = triplets(counts, idx, val)
    return float(np.bincount(r, np.abs(v), minlength=len(counts)).max())


# -------------------------------------------------------------------------------------------------------------- exact matvec
def _two_product(a, b):
    """p + e == a * b exactly (p the rounded product)"""
    p = a * b
    def split(x):
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi
    ah, al = split(a); bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_matvec(counts, idx, val, x):
    """(exact, sum_abs, length): per row the correctly rounded sum_j a_ij x_j, the correctly rounded sum_j |a_ij x_j| and the
    number of entries of the full row (stored zeros count: the kernel adds them too)"""
    n = len(counts)
    x = np.asarray(x, np.float64)
    r, c, v = triplets(counts, idx, val)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(v))
    p, e = _two_product(v, x[c])
    big = np.abs(p) > 1e-280
    assert np.all(np.abs(p) < 1e280) and np.all(p[~big] == 0.0), "two-product is exact only away from over- and underflow"
    order = np.argsort(r, kind="stable")
    r, p, e = r[order], p[order], e[order]
    sgn = np.where(np.signbit(p), -1.0, 1.0)
    ap, ae = sgn * p, sgn * e
    length = np.bincount(r, minlength=n)
    ends = np.cumsum(length)
    exact = np.zeros(n); sabs = np.zeros(n)
    b = 0
    for i in range(n):
        f = ends[i]
        if f - b == 1:
            exact[i] = p[b]; sabs[i] = ap[b]          # p is the correctly rounded single product
        elif f > b:
            exact[i] = math.fsum(p[b:f].tolist() + e[b:f].tolist())
            sabs[i] = math.fsum(ap[b:f].tolist() + ae[b:f].tolist())
        b = f
    return exact, sabs, length


def matvec_bound(sabs, length):
    """gamma_{L+1} sum|a x|, rounded up by one part in 2^50 (the bound itself is computed in floating point)"""
    return gamma(np.asarray(length) + 1.0) * np.asarray(sabs) * (1.0 + 2.0 ** -50)


def matvec_violations(y, exact, sabs, length):
    """rows where |y - exact| exceeds the bound, or is not finite; every row is looked at"""
    y = np.asarray(y, np.float64)
    err = np.abs(y - exact)
    return np.flatnonzero(~(err <= matvec_bound(sabs, length)))


# ------------------------------------------------------------------------------------------------------ eigenvalue references
def eigh_dense(counts, idx, val):
    assert len(counts) <= 2000
    return np.linalg.eigh(dense(counts, idx, val))


def arrow_lowest(d, b):
    """the lowest eigenvalue of the arrow matrix (diagonal d, A[0, i] = A[i, 0] = b[i], b[0] ignored) among those whose vector
    has weight on row 0: the lowest root of f(l) = d_0 - l - sum_i b_i^2 / (d_i - l), which falls monotonically from +inf to
    -inf below the smallest coupled d_i.  Bisection in long double."""
    d = np.asarray(d, np.longdouble); b = np.asarray(b, np.longdouble)
    on = np.flatnonzero(b[1:] != 0) + 1
    if len(on) == 0:
        return float(d[0])
    dc, b2 = d[on], b[on] * b[on]
    hi = dc.min()
    lo = min(hi, d[0]) - np.sqrt(b2.sum()) - np.longdouble(1)
    f = lambda l: d[0] - l - (b2 / (dc - l)).sum()
    assert f(lo) > 0
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
    return float(lo + (hi - lo) / 2)


def arrow_vector(d, b, lam):
    """the unit eigenvector of the arrow matrix at the root lam: x_i = b_i x_0 / (lam - d_i)"""
    d = np.asarray(d, np.longdouble); b = np.asarray(b, np.longdouble)
    x = np.zeros(len(d), np.longdouble); x[0] = 1
    x[1:] = b[1:] / (np.longdouble(lam) - d[1:])
    return (x / np.sqrt((x * x).sum())).astype(np.float64)


def sturm_count(a, b, lam):
    """number of eigenvalues below lam of the symmetric tridiagonal matrix (diagonal a[n], off-diagonal b[n-1])"""
    lam = np.longdouble(lam)
    tiny = np.finfo(np.longdouble).tiny * np.longdouble(2.0 ** 200)
    q = np.longdouble(1); cnt = 0
    for i in range(len(a)):
        q = np.longdouble(a[i]) - lam - (np.longdouble(b[i - 1]) ** 2 / q if i else 0)
        if q == 0:
            q = -tiny
        cnt += q < 0
    return int(cnt)


def tridiagonal_eigenvalue(a, b, k=0):
    """the k-th (0-based, ascending) eigenvalue by bisection on the Sturm count, in long double"""
    a = np.asarray(a, np.longdouble); b = np.asarray(b, np.longdouble)
    r = np.abs(a).max() + 2 * (np.abs(b).max() if len(b) else 0) + 1
    lo, hi = -r, r
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        if sturm_count(a, b, mid) > k:
            hi = mid
        else:
            lo = mid
    return float(lo + (hi - lo) / 2)


def residual_parts(counts, idx, val, e, x):
    """(r, floor, h) of an eigenpair (e, x), all over || x ||_2.  r = || A x - e x ||_2 with the exact matvec, h = || A x ||_2.
    floor: what a double-precision evaluation of that residual may itself be off by.  An iteration in doubles sees its residual only
    through its own matvec, whose row i is off by up to gamma_{L_i + 1} sum_j |a_ij x_j| (the bound of the matvec above, any summation
    order); the product e x_i rounds once and the difference rounds once, each relative to at most sum_j |a_ij x_j| + |e x_i|.  Row i of
    the evaluated residual is therefore within gamma_{L_i + 2} sum_j |a_ij x_j| + 2 u |e x_i| of the true one, and the floor is the
    2-norm of these.  No solver can be asked to push its residual below what it can see of it."""
    x = np.asarray(x, np.float64)
    y, sabs, length = exact_matvec(counts, idx, val, x)
    nx = np.linalg.norm(x)
    floor = gamma(length + 2.0) * sabs + 2.0 * U * abs(e) * np.abs(x)
    return float(np.linalg.norm(y - e * x) / nx), float(np.linalg.norm(floor) / nx), float(np.linalg.norm(y) / nx)


def residual(counts, idx, val, e, x):
    """|| A x - e x ||_2 / || x ||_2 with the exact matvec"""
    return residual_parts(counts, idx, val, e, x)[0]


def eigenvalue_slack(n, a_norm1):
    """what LAPACK's (or a bisection's) eigenvalues themselves may be off by: n 2^-52 ||A||_1"""
    return n * 2.0 ** -52 * a_norm1


# ---------------------------------------------------------------------------------------------------------------- generators
def random_sparse(n, seed, per_row=6.0, shift=0.0):
    """symmetric, about per_row off-diagonal entries per row at random places, N(0,1) values, diagonal N(0,1) + shift * i"""
    rng = np.random.default_rng(seed)
    ent = {(i, i): float(rng.standard_normal() + shift * i) for i in range(n)}
    m = int(min(per_row * n / 2, n * (n - 1) / 2))
    while m > 0 and n > 1:
        i, j = (int(t) for t in rng.integers(0, n, 2))
        if i != j and (i, j) not in ent and (j, i) not in ent:
            ent[(i, j)] = float(rng.standard_normal()); m -= 1
    return storage(n, ent)


def banded(n, bw, seed):
    rng = np.random.default_rng(seed)
    ent = {(i, i): float(rng.standard_normal()) for i in range(n)}
    for i in range(n):
        for j in range(max(0, i - bw), i):
            ent[(i, j)] = float(rng.standard_normal())
    return storage(n, ent)


def arrow(d, b):
    """diagonal d, couplings b[i] (i >= 1) to row 0 only; built without a dictionary: n may be 300 001"""
    d = np.asarray(d, np.float64); b = np.asarray(b, np.float64)
    n = len(d)
    counts = np.full(n, 2, np.int64); counts[0] = 1
    idx = np.ones(2 * n - 1, np.int64); val = np.zeros(2 * n - 1)
    idx[0] = 1; val[0] = d[0]
    idx[1::2] = np.arange(2, n + 1); val[1::2] = d[1:]
    idx[2::2] = 1; val[2::2] = b[1:]
    return counts, idx, val


def arrow_random(n, seed, coupling=0.3):
    """(d, b): d_0 = -1 below d_i in [0, 4), couplings N(0, coupling^2 / n) so that the shift of the lowest root is O(coupling^2)"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 4.0, n); d[0] = -1.0
    b = rng.standard_normal(n) * coupling / math.sqrt(n); b[0] = 0.0
    return d, b


def tridiagonal(a, b):
    n = len(a)
    counts = np.full(n, 2, np.int64); counts[0] = 1
    idx = np.ones(2 * n - 1, np.int64); val = np.zeros(2 * n - 1)
    val[0] = a[0]
    idx[1::2] = np.arange(2, n + 1); val[1::2] = np.asarray(a)[1:]
    idx[2::2] = np.arange(1, n); val[2::2] = np.asarray(b)
    return counts, idx, val


def diagonal(d):
    d = np.asarray(d, np.float64)
    return np.ones(len(d), np.int64), np.arange(1, len(d) + 1, dtype=np.int64), d.copy()


def block_diagonal(blocks):
    n = sum(len(B) for B in blocks)
    A = np.zeros((n, n)); o = 0
    for B in blocks:
        A[o:o + len(B), o:o + len(B)] = B; o += len(B)
    return storage_from_dense(A)


def random_symmetric(n, seed, dominance=3.0):
    """dense symmetric N(0,1) + N(0,1)^T with dominance * i added to the diagonal: diagonally dominant from the first rows on"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B + B.T + np.diag(np.arange(n) * dominance)


def row_length_ladder(seed):
    """full-row lengths LADDER: one isolated row, and hubs of length L = diagonal + (L - 1) leaves, each leaf a row of length 2;
    the rows are shuffled, so a hub's entries lie partly in its stored part and partly in the transposed part"""
    rng = np.random.default_rng(seed)
    hubs = [L for L in LADDER if L > 2]
    n = 1 + sum(hubs)                                # one isolated row + each hub with its L - 1 leaves
    perm = rng.permutation(n)
    ent = {(int(i), int(i)): float(rng.standard_normal()) for i in range(n)}
    at = 1
    for L in hubs:
        h = int(perm[at])
        for q in range(1, L):
            ent[(h, int(perm[at + q]))] = float(rng.standard_normal())
        at += L
    return storage(n, ent)


def cancellation(length):
    """row 0 of full length `length`: diagonal 1, then +1e16, -1e16, 1, +1e16, -1e16, 1, ...; x of ones.  The exact row sum is
    small, sum|a x| is about length/3 * 2e16: any summation order passes the bound, a dropped or doubled entry does not."""
    n = length
    ent = {(i, i): 1.0 for i in range(n)}
    for j in range(1, n):
        ent[(0, j)] = (1e16, -1e16, 1.0)[(j - 1) % 3]
    return storage(n, ent) + (np.ones(n),)


def stored_zeros(n, seed):
    """random sparse with a third of the stored values (diagonals included) replaced by 0.0 and -0.0"""
    c, i, v = random_sparse(n, seed)
    rng = np.random.default_rng(seed + 1)
    z = rng.random(len(v))
    v = np.where(z < 1 / 6, 0.0, np.where(z < 1 / 3, -0.0, v))
    return c, i, v


def generators(seed=2024):
    """name -> (counts, idx, val, x): every generator once, seeded"""
    rng = np.random.default_rng(seed)
    out = {}
    def put(name, cis, x=None):
        out[name] = tuple(cis) + ((rng.standard_normal(len(cis[0])) if x is None else x),)
    put("random_sparse", random_sparse(500, seed + 1))
    put("banded", banded(300, 70, seed + 2))
    put("arrow", arrow(*arrow_random(1000, seed + 3)))
    put("diagonal", diagonal(rng.standard_normal(129)))
    put("block_diagonal", block_diagonal([random_symmetric(m, seed + 4 + m) for m in (1, 3, 64, 65, 2)]))
    put("row_length_ladder", row_length_ladder(seed + 5))
    for L in (4, 65, 130):
        c, i, v, x = cancellation(L)
        put("cancellation_%d" % L, (c, i, v), x)
    put("stored_zeros", stored_zeros(200, seed + 6))
    return out


SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)


def sized(n, seed=77):
    c, i, v = random_sparse(n, seed + n, per_row=min(8.0, max(n - 1, 0)))
    return c, i, v, np.random.default_rng(seed + 1000 + n).standard_normal(n)
