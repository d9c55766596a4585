"""NumPy FP64 restatement of the sparse GP under k(x, x') = k_cov(x, x') + sum_e v_e x_e x'_e (include/cimrgp_sparse_linear.h,
DESIGN.md "A linear term for the sparse GP"), shared by tests/test_sparse_linear_host.py and the GPU tests.  The fit, the
prediction and the objective are written twice: by the Woodbury chain the device runs, and from the dense n x n definition
K~ = Q_ff + Lambda.  The gradient w.r.t. every parameter and Z is torch FP64 CPU autograd of the DENSE definition, so it
shares no step with the chain rule the device follows; autograd of the Woodbury chain is its second form, and the gap
between the two is the oracle's own error.  ``ell``: a scalar (isotropic) or a (d,) vector (ARD); ``lin``: the
(d,) variances v in the units of x; theta = (log sf, log l (1 or d), log noise, log v_1 .. log v_d).  Covariance ids are
those of include/cimrgp.h; mode 0 = FITC, 1 = VFE."""
import numpy as np
import scipy.linalg as sla

import sparse_ard_numpy as sa
import sparse_grad_numpy as sg
from grad_numpy import kcov


def ksum(xa, xb, cov, ell, sf2, lin):
    """k_cov(xa, xb) + sum_e lin_e xa_e xb_e.  A scalar ``ell`` goes to grad_numpy.kcov as it is (with lin = 0 the result is
    kcov's bit for bit); a vector divides the inputs and the covariance runs at unit length-scale."""
    lin = np.asarray(lin, dtype=np.float64)
    if np.ndim(ell) == 0:
        k = kcov(xa, xb, cov, ell, sf2)
    else:
        ell = np.asarray(ell, dtype=np.float64)
        k = kcov(xa / ell, xb / ell, cov, 1.0, sf2)
    return k + (xa * lin) @ xb.T


def kdiag(x, sf2, lin):
    """k(x_i, x_i) = sf2 + sum_e lin_e x_ie^2."""
    return sf2 + (x * x * np.asarray(lin, dtype=np.float64)).sum(axis=1)


def woodbury(x, z, r, cov, ell, sf2, noise, eps, mode, lin, xs=None, include_noise=False):
    """(lml, mean*, var*) by the chain of tests/sparse_numpy.woodbury, statement for statement, with the sum kernel and its
    diagonal; the jitter stays eps sf2 I."""
    n, q = r.shape
    m = z.shape[0]
    lu = np.linalg.cholesky(ksum(z, z, cov, ell, sf2, lin) + eps * sf2 * np.eye(m))
    a = sla.solve_triangular(lu, ksum(x, z, cov, ell, sf2, lin).T, lower=True).T
    qd = (a * a).sum(axis=1)
    kd = kdiag(x, sf2, lin)
    lam = (kd - qd + noise) if mode == 0 else np.full(n, float(noise))
    if not (lam > 0).all():
        raise np.linalg.LinAlgError("lambda not positive")
    aw = a / lam[:, None]
    lb = np.linalg.cholesky(np.eye(m) + a.T @ aw)
    gamma = sla.solve_triangular(lb, aw.T @ r, lower=True)
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * np.log(lam).sum() - q * np.log(np.diag(lb)).sum()
           - 0.5 * (r * r / lam[:, None]).sum() + 0.5 * (gamma * gamma).sum())
    if mode == 1:
        lml -= 0.5 * q * (kd - qd).sum() / noise
    if xs is None:
        return lml, None, None
    as_ = sla.solve_triangular(lu, ksum(xs, z, cov, ell, sf2, lin).T, lower=True).T
    ws = sla.solve_triangular(lb, as_.T, lower=True).T
    var = kdiag(xs, sf2, lin) - (as_ * as_).sum(axis=1) + (ws * ws).sum(axis=1) + (noise if include_noise else 0.0)
    return lml, ws @ gamma, var


def dense(x, z, r, cov, ell, sf2, noise, eps, mode, lin, xs=None, include_noise=False):
    """The same from the definition: K~ = Q_ff + Lambda (n x n), Q = K_.u (K_uu + eps sf I)^-1 K_u.; LML = log N(r | 0, K~)
    (- the trace term for VFE); mean* = Q_*f K~^-1 r, var* = k_** - Q_*f K~^-1 Q_f* (Q_** cancels)."""
    n, q = r.shape
    kuu = ksum(z, z, cov, ell, sf2, lin) + eps * sf2 * np.eye(z.shape[0])
    kfu = ksum(x, z, cov, ell, sf2, lin)
    qff = kfu @ np.linalg.solve(kuu, kfu.T)
    qd = np.diag(qff)
    kd = kdiag(x, sf2, lin)
    lam = (kd - qd + noise) if mode == 0 else np.full(n, float(noise))
    lt = np.linalg.cholesky(qff + np.diag(lam))
    alpha = sla.cho_solve((lt, True), r)
    lml = -0.5 * n * q * np.log(2 * np.pi) - q * np.log(np.diag(lt)).sum() - 0.5 * (r * alpha).sum()
    if mode == 1:
        lml -= 0.5 * q * (kd - qd).sum() / noise
    if xs is None:
        return lml, None, None
    qsf = ksum(xs, z, cov, ell, sf2, lin) @ np.linalg.solve(kuu, kfu.T)
    v = sla.solve_triangular(lt, qsf.T, lower=True)
    var = kdiag(xs, sf2, lin) - (v * v).sum(axis=0) + (noise if include_noise else 0.0)
    return lml, qsf @ alpha, var


def _theta(ell, sf2, noise, lin):
    return np.log(np.concatenate([[sf2], np.atleast_1d(np.asarray(ell, dtype=np.float64)), [noise], np.asarray(lin, dtype=np.float64)]))


def grad_dense(x, z, r, cov, ell, sf2, noise, eps, mode, lin, want_z=True):
    """(lml, dtheta, dZ or None) by torch FP64 CPU autograd of the DENSE definition (an n x n Cholesky)."""
    import torch
    n, q = r.shape
    m, d = z.shape
    ne = np.size(ell)
    theta = torch.tensor(_theta(ell, sf2, noise, lin), dtype=torch.float64, requires_grad=True)
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=bool(want_z))
    xt, rt = torch.tensor(np.asarray(x, dtype=np.float64)), torch.tensor(np.asarray(r, dtype=np.float64))
    sf, el, s2, v = torch.exp(theta[0]), torch.exp(theta[1:1 + ne]), torch.exp(theta[1 + ne]), torch.exp(theta[2 + ne:])

    def k(a, b):
        return sg._kcov_torch(torch, a / el, b / el, cov, 1.0, sf) + (a * v) @ b.T

    kuu = k(zt, zt) + eps * sf * torch.eye(m, dtype=torch.float64)
    kfu = k(xt, zt)
    qff = kfu @ torch.linalg.solve(kuu, kfu.T)
    qd = torch.diagonal(qff)
    kd = sf + (xt * xt * v).sum(dim=1)
    lam = (kd - qd + s2) if mode == 0 else s2 * torch.ones(n, dtype=torch.float64)
    lt = torch.linalg.cholesky(qff + torch.diag(lam))
    alpha = torch.cholesky_solve(rt, lt)
    lml = -0.5 * n * q * np.log(2 * np.pi) - q * torch.log(torch.diagonal(lt)).sum() - 0.5 * (rt * alpha).sum()
    if mode == 1:
        lml = lml - 0.5 * q * (kd - qd).sum() / s2
    lml.backward()
    return float(lml.item()), theta.grad.numpy().copy(), (zt.grad.numpy().copy() if want_z else None)


def grad_woodbury(x, z, r, cov, ell, sf2, noise, eps, mode, lin, want_z=True):
    """(lml, dtheta, dZ or None) by torch FP64 CPU autograd of the Woodbury chain: the second form of the gradient.  Its gap
    to :func:`grad_dense` on the same inputs is the oracle's own error, which grows with cond(K_uu + eps sf I)."""
    import torch
    n, q = r.shape
    m, d = z.shape
    ne = np.size(ell)
    theta = torch.tensor(_theta(ell, sf2, noise, lin), dtype=torch.float64, requires_grad=True)
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=bool(want_z))
    xt, rt = torch.tensor(np.asarray(x, dtype=np.float64)), torch.tensor(np.asarray(r, dtype=np.float64))
    sf, el, s2, v = torch.exp(theta[0]), torch.exp(theta[1:1 + ne]), torch.exp(theta[1 + ne]), torch.exp(theta[2 + ne:])

    def k(a, b):
        return sg._kcov_torch(torch, a / el, b / el, cov, 1.0, sf) + (a * v) @ b.T

    eye = torch.eye(m, dtype=torch.float64)
    lu = torch.linalg.cholesky(k(zt, zt) + eps * sf * eye)
    a = torch.linalg.solve_triangular(lu, k(xt, zt).T, upper=False).T
    qd = (a * a).sum(dim=1)
    kd = sf + (xt * xt * v).sum(dim=1)
    lam = (kd - qd + s2) if mode == 0 else s2 * torch.ones(n, dtype=torch.float64)
    aw = a / lam[:, None]
    lb = torch.linalg.cholesky(eye + a.T @ aw)
    gamma = torch.linalg.solve_triangular(lb, aw.T @ rt, upper=False)
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * torch.log(lam).sum() - q * torch.log(torch.diagonal(lb)).sum()
           - 0.5 * (rt * rt / lam[:, None]).sum() + 0.5 * (gamma * gamma).sum())
    if mode == 1:
        lml = lml - 0.5 * q * (kd - qd).sum() / s2
    lml.backward()
    return float(lml.item()), theta.grad.numpy().copy(), (zt.grad.numpy().copy() if want_z else None)


def central(x, z, r, cov, ell, sf2, noise, eps, mode, lin, step=1e-5, want_z_rows=()):
    """Central differences of :func:`woodbury`: (dtheta, {(j, e): dF / dz_je for the rows j of ``want_z_rows``})."""
    ne, d = np.size(ell), z.shape[1]
    th0 = _theta(ell, sf2, noise, lin)

    def f(th, zz):
        v = np.exp(th)
        el = float(v[1]) if np.ndim(ell) == 0 else v[1:1 + ne]
        return woodbury(x, zz, r, cov, el, v[0], v[1 + ne], eps, mode, v[2 + ne:])[0]

    out = np.empty(th0.shape[0])
    for k in range(th0.shape[0]):
        hi, lo = th0.copy(), th0.copy()
        hi[k] += step
        lo[k] -= step
        out[k] = (f(hi, z) - f(lo, z)) / (2 * step)
    dz = {}
    for j in want_z_rows:
        for e in range(d):
            hi, lo = z.copy(), z.copy()
            hi[j, e] += step
            lo[j, e] -= step
            dz[(j, e)] = (f(th0, hi) - f(th0, lo)) / (2 * step)
    return out, dz


def pair_grad_lin(xa, xb, g, cov, ell, sf2, lin, ard, scale=1.0, ft=np.float64):
    """The contraction of cimrgp_cov_pair_grad_lin evaluated in the float type ``ft``:
    ((sums, lsums (d,), db (nb x d), the linear share of db), (sums of magnitudes of the terms of sums, lsums, db's linear share)).
    ``sums``: the twin's, [sum G k, sum G dk/dlog l] or, with ``ard``, sparse_ard_numpy.pair_grad_ard's 1 + d."""
    d = xa.shape[1]
    (s_ard, db_cov), (m_ard, _) = sa.pair_grad_ard(xa, xb, g, cov, ell, sf2, scale, ft)
    sums = s_ard if ard else np.array([s_ard[0], s_ard[1:].sum()])
    smag = m_ard if ard else np.array([m_ard[0], m_ard[1:].sum()])
    gl, al, bl = np.asarray(g, dtype=ft), np.asarray(xa, dtype=ft), np.asarray(xb, dtype=ft)
    p = gl.T @ al                                        # nb x d
    pmag = np.abs(gl).T @ np.abs(al)
    lsums = np.array((bl * p).sum(axis=0), dtype=np.float64)
    lmag = np.array((np.abs(bl) * pmag).sum(axis=0), dtype=np.float64)
    lin = np.asarray(lin, dtype=ft)
    db_lin = np.array(ft(scale) * lin * p, dtype=np.float64)
    db_lin_mag = np.array(abs(ft(scale)) * np.abs(lin) * pmag, dtype=np.float64)
    return (sums, lsums, db_cov + db_lin, db_lin), (smag, lmag, db_lin_mag)


def pair_scratch_bytes(na, nb, d, ard):
    """cimrgp_cov_pair_grad_lin_scratch_bytes by its formula: the twin's plus a second partial array of the partial db's size."""
    twin = sa.pair_scratch_bytes(na, nb, d) if ard else sg.pair_scratch_bytes(na, nb, d)
    return twin + 8 * sg.pair_slices(na, nb)[0] * ((nb + 127) // 128) * 128 * d


def trend_problem(n, seed):
    """The extrapolation case: y = 1.5 x0 + sin(3 x0) + 0.1 noise on x0 in [-1, 1]; (x (n x 1), y (n x 1), target(x0))."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-1.0, 1.0, size=(n, 1)), axis=0)

    def target(t):
        return 1.5 * t + np.sin(3.0 * t)

    return x, target(x) + 0.1 * rng.normal(size=(n, 1)), target
