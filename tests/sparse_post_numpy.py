"""NumPy restatement of the sparse GP's posterior queries (include/cimrgp_sparse_post.h, DESIGN.md "Posterior queries of the
sparse GP"), shared by tests/test_sparse_post_host.py and the GPU tests.  Two independent forms, as in sparse_numpy.py: the
Woodbury chain the device runs, and the dense n x n definition K~ = Q_ff + Lambda.  Covariance ids are those of
include/cimrgp.h; mode 0 = FITC, 1 = VFE."""
import numpy as np
import scipy.linalg as sla

from grad_numpy import central_diff, g_of, kcov, rel  # noqa: F401
from sparse_numpy import _a_of, _chol_uu, problem, woodbury  # noqa: F401


class Fit(object):
    """What stays after a sparse fit (the Woodbury chain of sparse_numpy.woodbury): L_u, A, lambda, L_B, gamma."""

    def __init__(self, x, z, r, cov, ell, sf2, noise, eps, mode):
        self.x, self.z, self.r, self.cov, self.ell, self.sf2, self.noise, self.mode = x, z, r, cov, ell, sf2, noise, mode
        n, m = x.shape[0], z.shape[0]
        self.lu = _chol_uu(z, cov, ell, sf2, eps)
        self.a = _a_of(x, z, self.lu, cov, ell, sf2)
        qd = (self.a * self.a).sum(axis=1)
        self.lam = (sf2 - qd + noise) if mode == 0 else np.full(n, float(noise))
        aw = self.a / self.lam[:, None]
        self.lb = np.linalg.cholesky(np.eye(m) + self.a.T @ aw)
        self.gamma = sla.solve_triangular(self.lb, aw.T @ r, lower=True)

    def rows(self, k):
        """(A*, W*) of the rows k = K(., Z) (any stack of rows: the solves act row by row)."""
        a = sla.solve_triangular(self.lu, k.T, lower=True).T
        return a, sla.solve_triangular(self.lb, a.T, lower=True).T

    def star(self, xs):
        return self.rows(kcov(xs, self.z, self.cov, self.ell, self.sf2))


def cross_grad(xa, xb, cov, ell, sf2):
    """The d + 1 slabs of cimrgp_cov_cross_grad: K(xa, xb), then dK / d xa_e = -g (xa_e - xb_e)."""
    g = g_of(xa, xb, cov, ell, sf2)
    diff = xa[:, None, :] - xb[None, :, :]
    return np.concatenate([kcov(xa, xb, cov, ell, sf2)[None], np.moveaxis(-g[:, :, None] * diff, 2, 0)], axis=0)


def tail_grad(aslabs, wslabs, gamma):
    """(mean_grad (ns, d, q), var_grad (ns, d)) and the sums of magnitudes their componentwise bounds scale with."""
    a0, da, w0, dw = aslabs[0], aslabs[1:], wslabs[0], wslabs[1:]
    mg = np.einsum('eij,jc->iec', dw, gamma)
    vg = 2.0 * np.einsum('eij,ij->ie', dw, w0) - 2.0 * np.einsum('eij,ij->ie', da, a0)
    mg_mag = np.einsum('eij,jc->iec', np.abs(dw), np.abs(gamma))
    vg_mag = 2.0 * np.einsum('eij,ij->ie', np.abs(dw), np.abs(w0)) + 2.0 * np.einsum('eij,ij->ie', np.abs(da), np.abs(a0))
    return mg, vg, mg_mag, vg_mag


def predict_grad(fit, xs):
    """Woodbury: the stacked slabs through the two row solves."""
    ns, d = xs.shape
    m = fit.z.shape[0]
    slabs = cross_grad(xs, fit.z, fit.cov, fit.ell, fit.sf2)
    a, w = fit.rows(slabs.reshape((d + 1) * ns, m))
    return tail_grad(a.reshape(d + 1, ns, m), w.reshape(d + 1, ns, m), fit.gamma)[:2]


def predict_grad_alpha(fit, xs):
    """The shorter route the device does NOT take: weights alpha = L_u^-T L_B^-T gamma against the raw derivative slabs."""
    alpha = sla.solve_triangular(fit.lu.T, sla.solve_triangular(fit.lb.T, fit.gamma, lower=False), lower=False)
    slabs = cross_grad(xs, fit.z, fit.cov, fit.ell, fit.sf2)
    return np.einsum('eij,jc->iec', slabs[1:], alpha)


def loo_rows(a, v, gamma, r, sf2, noise, mode):
    """cimrgp_sparse_loo per row: (loo_mean, loo_var, h, magnitudes of the sums behind mu and |V_i|^2)."""
    lam = (sf2 - (a * a).sum(axis=1) + noise) if mode == 0 else np.full(a.shape[0], float(noise))
    h = (v * v).sum(axis=1) / lam
    mu = v @ gamma
    return r - (r - mu) / (1.0 - h)[:, None], lam / (1.0 - h), h, np.abs(v) @ np.abs(gamma), lam


def loo(fit):
    """Woodbury: (loo_mean (n, q), loo_var (n,), h (n,))."""
    v = sla.solve_triangular(fit.lb, fit.a.T, lower=True).T
    return loo_rows(fit.a, v, fit.gamma, fit.r, fit.sf2, fit.noise, fit.mode)[:3]


def _dense_parts(fit):
    kuu = fit.lu @ fit.lu.T
    kfu = kcov(fit.x, fit.z, fit.cov, fit.ell, fit.sf2)
    qff = kfu @ np.linalg.solve(kuu, kfu.T)
    lam = (fit.sf2 - np.diag(qff) + fit.noise) if fit.mode == 0 else np.full(fit.x.shape[0], float(fit.noise))
    return kuu, kfu, qff + np.diag(lam)


def loo_dense(fit):
    """From the definition: K~^-1 (n x n); mean_i = r_i - [K~^-1 r]_i / [K~^-1]_ii, var_i = 1 / [K~^-1]_ii."""
    _, _, kt = _dense_parts(fit)
    kinv = np.linalg.inv(kt)
    kinv = 0.5 * (kinv + kinv.T)
    dg = np.diag(kinv)
    return fit.r - (kinv @ fit.r) / dg[:, None], 1.0 / dg


def joint_cov(fit, xs, diag=0.0):
    """Woodbury: (Sigma, the magnitudes sum_k |A A| + |W W|, |K**|)."""
    a, w = fit.star(xs)
    kss = kcov(xs, xs, fit.cov, fit.ell, fit.sf2)
    return (kss + diag * np.eye(xs.shape[0]) - a @ a.T + w @ w.T, np.abs(a) @ np.abs(a).T + np.abs(w) @ np.abs(w).T,
            np.abs(kss) + abs(diag) * np.eye(xs.shape[0]))


def joint_cov_dense(fit, xs):
    """From the definition: Q*f K~^-1 Qf* subtracted from Q**, plus K** - Q**."""
    kuu, kfu, kt = _dense_parts(fit)
    ksu = kcov(xs, fit.z, fit.cov, fit.ell, fit.sf2)
    qsf = ksu @ np.linalg.solve(kuu, kfu.T)
    qss = ksu @ np.linalg.solve(kuu, ksu.T)
    kss = kcov(xs, xs, fit.cov, fit.ell, fit.sf2)
    return qss - qsf @ np.linalg.solve(kt, qsf.T) + (kss - qss)


def predict_grad_dense(fit, xs):
    """From the definition: mean* = Q*f K~^-1 r = K*u beta and var* = sf - Q*f K~^-1 Qf* = sf - K*u P Ku* with
    S = Kuu^-1 Kuf, beta = S K~^-1 r and P = S K~^-1 S^T, differentiated through K*u alone."""
    kuu, kfu, kt = _dense_parts(fit)
    s = np.linalg.solve(kuu, kfu.T)                          # Kuu^-1 Kuf (m x n)
    beta = s @ np.linalg.solve(kt, fit.r)
    p = s @ np.linalg.solve(kt, s.T)
    slabs = cross_grad(xs, fit.z, fit.cov, fit.ell, fit.sf2)
    return np.einsum('eij,jc->iec', slabs[1:], beta), -2.0 * np.einsum('eij,ij->ie', slabs[1:], slabs[0] @ p)


def central(fit, xs, h=1e-5):
    """Central differences of the Woodbury prediction: (dmean (ns, d, q), dvar (ns, d))."""
    def f(p):
        a, w = fit.star(p)
        return w @ fit.gamma, fit.sf2 - (a * a).sum(axis=1) + (w * w).sum(axis=1)
    return central_diff(f, xs, h)
