"""NumPy restatement of the leave-one-out cross-validation (include/cimrgp_loo.h, DESIGN.md "Leave-one-out
cross-validation"), shared by tests/test_loo_host.py and the GPU tests.  Covariance ids are those of include/cimrgp.h
(CIMRGP_COV_*)."""
import numpy as np
import scipy.linalg as sla

from grad_numpy import kcov, rel  # noqa: F401  (rel is re-exported)


def trtri(lower):
    """U = L^-T (upper triangular) by a triangular solve."""
    n = lower.shape[0]
    return sla.solve_triangular(lower, np.eye(n), lower=True).T


def kinv_diag(lower):
    """diag(K^-1) = squared row norms of L^-T."""
    return (trtri(lower) ** 2).sum(axis=1)


def loo_closed_form(K, y, r):
    """(mean (n, q), var (n,)) of y_i predicted from the other points of the block: K (noise included), observations y,
    residual targets r = y - f_bar - bias."""
    lower = np.linalg.cholesky(K)
    alpha = sla.cho_solve((lower, True), r)
    d = kinv_diag(lower)
    return y - alpha / d[:, None], 1.0 / d


def loo_brute_force(K, y, r, points=None):
    """The same by refits: delete point i, solve again, predict y_i (the prior mean f_bar_i + bias = y_i - r_i is known
    at the withheld point)."""
    n = K.shape[0]
    points = range(n) if points is None else points
    mean, var = [], []
    for i in points:
        keep = np.arange(n) != i
        Kk = K[np.ix_(keep, keep)]
        ki = K[keep, i]
        sol = np.linalg.solve(Kk, np.column_stack([r[keep], ki]))
        mean.append(y[i] - r[i] + ki @ sol[:, :-1])
        var.append(K[i, i] - ki @ sol[:, -1])
    return np.array(mean), np.array(var)


def loo_log_density(y, mean, var):
    """(n,) Gaussian log densities of y under N(mean, var I), summed over the outputs."""
    q = y.shape[1]
    return -0.5 * q * np.log(2 * np.pi * var) - 0.5 * ((y - mean) ** 2).sum(axis=1) / var


def scratch_bytes(esz, n, strip_rows):
    """cimrgp_kinv_diag_scratch_bytes by its formula."""
    top = (n + 255) // 256 * 256
    strip = 256 if strip_rows < 256 else min(top, (strip_rows + 255) // 256 * 256)
    return strip * ((n + 15) // 16 * 16) * esz
