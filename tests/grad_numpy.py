"""NumPy restatement of the predictive gradients (include/cimrgp_grad.h, DESIGN.md "Predictive gradients"), shared by
tests/test_grad_host.py and tests/test_gpu_grad.py.  Covariance ids are those of include/cimrgp.h (CIMRGP_COV_*)."""
import numpy as np

NU = {1: 0.5, 2: 1.5, 3: 2.5}


def kcov(xa, xb, cov, ell, sf2):
    """k(xa_i, xb_j) of covariance ``cov``."""
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    if cov == 0:
        return sf2 * np.exp(-0.5 * d2 / ell ** 2)
    t = np.sqrt(2 * NU[cov]) * np.sqrt(d2) / ell
    poly = {1: 1.0, 2: 1 + t, 3: 1 + t + t * t / 3}[cov]
    return sf2 * poly * np.exp(-t)


def g_of(xa, xb, cov, ell, sf2):
    """g(r_ij) with dk(xa_i, xb_j)/dxa_ie = -g_ij (xa_ie - xb_je); Matern 1/2 takes 0 at r = 0."""
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    r = np.sqrt(d2)
    if cov == 0:
        return sf2 / ell ** 2 * np.exp(-0.5 * d2 / ell ** 2)
    if cov == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, sf2 / (ell * np.where(r > 0, r, 1.0)) * np.exp(-r / ell), 0.0)
    if cov == 2:
        return 3 * sf2 / ell ** 2 * np.exp(-np.sqrt(3) * r / ell)
    return 5 * sf2 / (3 * ell ** 2) * (1 + np.sqrt(5) * r / ell) * np.exp(-np.sqrt(5) * r / ell)


def contract(x, alpha, xs, cov, ell, sf2, beta=None):
    """(mean_grad (ns, d, q), var_grad (ns, d) or None): the contraction of cimrgp_cov_predict_grad."""
    g = g_of(xs, x, cov, ell, sf2)                           # (ns, n)
    diff = xs[:, None, :] - x[None, :, :]                    # (ns, n, d)
    mg = -np.einsum("ij,ije,jc->iec", g, diff, alpha)
    vg = None if beta is None else 2 * np.einsum("ij,ij,ije->ie", beta, g, diff)
    return mg, vg


def block_grad(x, r, xs, cov, ell, sf2, noise):
    """Gradients of one block fitted on targets r (n x q) with K = k(x, x) + noise I."""
    K = kcov(x, x, cov, ell, sf2) + noise * np.eye(x.shape[0])
    alpha = np.linalg.solve(K, r)
    beta = np.linalg.solve(K, kcov(xs, x, cov, ell, sf2).T).T
    return contract(x, alpha, xs, cov, ell, sf2, beta)


def block_mean_var(x, r, xs, cov, ell, sf2, noise):
    K = kcov(x, x, cov, ell, sf2) + noise * np.eye(x.shape[0])
    ks = kcov(xs, x, cov, ell, sf2)
    mean = ks @ np.linalg.solve(K, r)
    var = sf2 - np.einsum("ij,ij->i", ks, np.linalg.solve(K, ks.T).T)
    return mean, var


def central_diff(f, xs, h):
    """Central differences of f(xs) -> (mean (ns, q), var (ns,)) per input dimension, every row perturbed at once (each
    row's prediction depends on its own row only): (dmean (ns, d, q), dvar (ns, d))."""
    ns, d = xs.shape
    dm, dv = None, np.zeros((ns, d))
    for e in range(d):
        xp, xm = xs.copy(), xs.copy()
        xp[:, e] += h
        xm[:, e] -= h
        mp, vp = f(xp)
        mm, vm = f(xm)
        if dm is None:
            dm = np.zeros((ns, d, mp.shape[1]))
        dm[:, e, :] = (mp - mm) / (2 * h)
        dv[:, e] = (vp - vm) / (2 * h)
    return dm, dv


def rel(a, b):
    """Largest absolute difference relative to the largest magnitude of the reference."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))
