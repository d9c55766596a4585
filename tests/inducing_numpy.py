"""NumPy restatement of the greedy inducing-point selection (include/cimrgp_inducing.h; DESIGN.md, "Greedy inducing-point
selection"): the pivoted Cholesky factorisation of K(X, X) stopped after m columns, with the device's rules -- d_i starts as
sf2 + sum_e lin_e x_ie^2, ties go to the lowest row, a NaN residual is never larger than anything, a pivot residual at or
below the floor leaves a zero column, picked rows are marked.  It runs in float64 or numpy.longdouble (``ft``), can be forced
along a given pivot sequence, and reports the top-two residual gap of every step.  Shared by tests/test_inducing_host.py and
the GPU tests.  Covariance ids are those of include/cimrgp.h."""
import numpy as np

LD = np.longdouble
COV_RBF, COV_MATERN12, COV_MATERN32, COV_MATERN52 = 0, 1, 2, 3
EPS = float(np.finfo(np.float64).eps)


def cov_matrix(xa, xb, cov, ell, sf2, lin=None, ft=np.float64):
    """k(xa_i, xb_j) = k_cov + sum_e lin_e xa_ie xb_je in the float type ``ft``."""
    xa, xb = np.asarray(xa, dtype=ft), np.asarray(xb, dtype=ft)
    ell, sf2 = ft(ell), ft(sf2)
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(axis=2)
    if cov == COV_RBF:
        k = sf2 * np.exp(-d2 / (2 * ell * ell))
    else:
        nu2 = {COV_MATERN12: 1, COV_MATERN32: 3, COV_MATERN52: 5}[cov]
        t = np.sqrt(ft(nu2)) * np.sqrt(d2) / ell
        poly = {COV_MATERN12: 1 + 0 * t, COV_MATERN32: 1 + t, COV_MATERN52: 1 + t + t * t / 3}[cov]
        k = sf2 * poly * np.exp(-t)
    if lin is not None:
        k = k + (xa * np.asarray(lin, dtype=ft)) @ xb.T
    return k


def start_diag(x, sf2, lin=None, ft=np.float64):
    x = np.asarray(x, dtype=ft)
    d = np.full(x.shape[0], ft(sf2), dtype=ft)
    return d if lin is None else d + (x * x * np.asarray(lin, dtype=ft)).sum(axis=1)


def pick(d, picked):
    """(arg-max of d over the rows not picked: lowest index on ties, a NaN never larger than anything; the largest and the
    second-largest value among them, the second -inf when one row is left)."""
    key = np.where(np.isnan(d), -np.inf, d).astype(d.dtype)
    key[picked] = -np.inf
    free = np.nonzero(~picked)[0]
    p = int(free[np.argmax(key[free])])          # argmax returns the first of equal values: the lowest row
    vals = np.sort(key[free])
    return p, vals[-1], (vals[-2] if vals.size > 1 else -np.inf)


def pivoted_cholesky(x, m, cov, ell, sf2, lin=None, floor=0.0, ft=np.float64, pivots=None, keep=False):
    """dict(pivots (m,), lt (m x n: row j is column j of L), diag (n,: -1 for picked rows), trace (m + 1,), rank, gaps (m,:
    largest minus second-largest residual among the rows not picked at each step), best (m,: the largest), at (m,: the
    residual of the row picked)).  ``pivots``: the sequence to follow in place of the arg-max (gaps / best still report the
    step's own residuals).  ``keep``: also ds (m x n), the residuals each step chose from (NaN for picked rows)."""
    x = np.asarray(x, dtype=ft)
    n = x.shape[0]
    d = start_diag(x, sf2, lin, ft)
    lt = np.zeros((m, n), dtype=ft)
    picked = np.zeros(n, dtype=bool)
    trace = np.zeros(m + 1, dtype=ft)
    trace[0] = d.sum()
    out_p, gaps, best, at = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=ft), np.zeros(m, dtype=ft), np.zeros(m, dtype=ft)
    rank, ds = 0, []
    for j in range(m):
        p, top, second = pick(d, picked)
        if keep:
            ds.append(np.where(picked, ft(np.nan), d))
        gaps[j], best[j] = top - second, top
        if pivots is not None:
            p = int(pivots[j])
            assert not picked[p], "forced pivot %d of step %d is already picked" % (p, j)
        out_p[j], at[j] = p, d[p]
        if d[p] > floor:
            rank += 1
            k = cov_matrix(x, x[p:p + 1], cov, ell, sf2, lin, ft)[:, 0]
            c = (k - lt[:j].T @ lt[:j, p]) / np.sqrt(d[p])
            lt[j] = c
            d = np.where(picked, d, d - c * c)
        picked[p] = True
        free = ~picked
        trace[j + 1] = np.maximum(d[free], 0).sum() if free.any() else 0
    diag = np.where(picked, ft(-1), d)
    return dict(pivots=out_p, lt=lt, diag=diag, trace=trace, rank=rank, gaps=gaps, best=best, at=at, ds=np.array(ds) if keep else None)


def nystrom_trace(x, rows, cov, ell, sf2, lin=None, ft=LD):
    """tr(K - K_xz K_zz^-1 K_zx) for Z = x[rows], by an unpivoted Cholesky factorisation of K_zz in ``ft``."""
    x = np.asarray(x, dtype=ft)
    z = x[np.asarray(rows)]
    kzz = cov_matrix(z, z, cov, ell, sf2, lin, ft)
    kxz = cov_matrix(x, z, cov, ell, sf2, lin, ft)
    m = z.shape[0]
    l = np.zeros((m, m), dtype=ft)
    for j in range(m):
        l[j, j] = np.sqrt(kzz[j, j] - (l[j, :j] ** 2).sum())
        l[j + 1:, j] = (kzz[j + 1:, j] - l[j + 1:, :j] @ l[j, :j]) / l[j, j]
    a = np.zeros_like(kxz)
    for j in range(m):                               # A = K_xz L^-T, column by column
        a[:, j] = (kxz[:, j] - a[:, :j] @ l[j, :j]) / l[j, j]
    return start_diag(x, sf2, lin, ft).sum() - (a * a).sum()


def qualifies(gaps, max_kii, stationary, m, n, rel=1e-9):
    """The gap condition under which the whole pivot sequence is asserted: the long-double top-two gap is >= rel * max K_ii
    at every step, step 0 of a stationary kernel without a linear term (an exact tie) and the last step of m = n (one row
    left) excluded."""
    g = np.asarray(gaps, dtype=np.float64).copy()
    keep = np.ones(g.shape[0], dtype=bool)
    if stationary:
        keep[0] = False
    if m == n:
        keep[-1] = False
    return bool((g[keep] >= rel * max_kii).all())


def clustered(n=3000, seed=0):
    """The clustered 1-D inputs of the quality check: 90 % of the rows from N(0, 0.05^2), the rest uniform on [-3, 3]."""
    rng = np.random.default_rng(seed)
    k = int(round(0.9 * n))
    x = np.concatenate([0.05 * rng.normal(size=k), rng.uniform(-3, 3, size=n - k)])
    return rng.permutation(x)[:, None]


def vfe_bound(x, y, rows, cov, ell, sf2, noise, eps=1e-6):
    """(Titsias' bound, tr(K - Q)) for Z = x[rows] on targets y (n x q), float64, K_uu + eps sf2 I as the device block forms it."""
    import scipy.linalg as sl
    n, q = y.shape
    z = x[np.asarray(rows)]
    m = z.shape[0]
    lu = np.linalg.cholesky(cov_matrix(z, z, cov, ell, sf2) + eps * sf2 * np.eye(m))
    a = sl.solve_triangular(lu, cov_matrix(x, z, cov, ell, sf2).T, lower=True).T
    lb = np.linalg.cholesky(np.eye(m) + a.T @ a / noise)
    gamma = sl.solve_triangular(lb, a.T @ y / noise, lower=True)
    slack = n * sf2 - (a * a).sum()
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * n * np.log(noise) - q * np.log(np.diag(lb)).sum()
           - 0.5 * (y * y).sum() / noise + 0.5 * (gamma * gamma).sum() - 0.5 * q * slack / noise)
    return float(lml), float(slack)
