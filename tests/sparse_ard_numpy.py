"""The sparse objective with one length-scale per input dimension (include/cimrgp_sparse_ard.h, DESIGN.md "ARD
length-scales for the sparse GP") in two independent forms, shared by tests/test_sparse_ard_host.py and the GPU tests: the
NumPy chain of tests/sparse_grad_numpy.py on pre-scaled inputs with the per-dimension pair sums written out, and torch FP64
CPU autograd of the Woodbury chain with a length-scale vector.  theta = (log sf, log l_1 .. log l_d, log noise); dZ is
w.r.t. Z in unscaled units."""
import numpy as np
import scipy.linalg as sla

import sparse_grad_numpy as sg
import sparse_numpy as sn
from grad_numpy import NU, kcov


def k_and_g(xa, xb, cov, ell, sf2, ft=np.float64):
    """(k, g, differences (na x nb x d)) of every pair, the formulae of grad_numpy.kcov / g_of evaluated in the float type
    ``ft`` (numpy.longdouble: so that the reference's own rounding does not spend the device's bound)."""
    xa, xb, ell, sf2 = np.asarray(xa, dtype=ft), np.asarray(xb, dtype=ft), ft(ell), ft(sf2)
    df = xa[:, None, :] - xb[None, :, :]
    d2 = (df * df).sum(-1)
    r = np.sqrt(d2)
    if cov == 0:
        k = sf2 * np.exp(-d2 / (2 * ell * ell))
        return k, k / (ell * ell), df
    t = np.sqrt(ft(2 * NU[cov])) * r / ell
    e = np.exp(-t)
    if cov == 1:
        return sf2 * e, np.where(r > 0, sf2 * e / (ell * np.where(r > 0, r, ft(1))), ft(0)), df
    if cov == 2:
        return sf2 * (1 + t) * e, 3 * sf2 / (ell * ell) * e, df
    return sf2 * (1 + t + t * t / 3) * e, 5 * sf2 / (3 * ell * ell) * (1 + t) * e, df


def pair_grad_ard(xa, xb, g, cov, ell, sf2, scale=1.0, ft=np.float64):
    """The contraction of cimrgp_cov_pair_grad_ard: ((sums (1 + d,), db (nb x d)), (sums of magnitudes of the same terms)),
    evaluated in ``ft`` and returned as float64."""
    d = xa.shape[1]
    k, gr, df = k_and_g(xa, xb, cov, ell, sf2, ft)
    g = np.asarray(g, dtype=ft)
    gk, gg = g * k, g * gr
    sums, smag = np.empty(1 + d), np.empty(1 + d)
    sums[0], smag[0] = gk.sum(), np.abs(gk).sum()
    db, mag = np.empty((xb.shape[0], d)), np.empty((xb.shape[0], d))
    for e in range(d):
        sq = gg * df[:, :, e] * df[:, :, e]
        sums[1 + e], smag[1 + e] = sq.sum(), np.abs(sq).sum()
        term = ft(scale) * gg * df[:, :, e]
        db[:, e], mag[:, e] = term.sum(axis=0), np.abs(term).sum(axis=0)
    return (sums, db), (smag, mag)


def chain(x, z, r, cov, ells, sf2, noise, eps, mode):
    """(lml, dtheta (d + 2,), dZ (m x d)): sparse_grad_numpy.chain on x / l, z / l at unit length-scale; the derivatives
    w.r.t. log l_e are the per-dimension pair sums of G_fu (K_fu's pairs) and G_uu (K_uu's), rebuilt from the chain's parts."""
    ells = np.asarray(ells, dtype=np.float64)
    xs, zs = x / ells, z / ells
    lml, dth, dzs, parts = sg.chain(xs, zs, r, cov, 1.0, sf2, noise, eps, mode)
    m = z.shape[0]
    lu = np.linalg.cholesky(kcov(zs, zs, cov, 1.0, sf2) + eps * sf2 * np.eye(m))
    gfu = sla.solve_triangular(lu.T, parts["ga"].T, lower=False).T
    guu = -0.5 * sla.solve_triangular(lu.T, sla.solve_triangular(lu.T, parts["M"], lower=False).T, lower=False)
    guu = 0.5 * (guu + guu.T)
    (s_fu, _), _ = pair_grad_ard(xs, zs, gfu, cov, 1.0, sf2)
    (s_uu, _), _ = pair_grad_ard(zs, zs, guu, cov, 1.0, sf2)
    return lml, np.concatenate([[dth[0]], s_fu[1:] + s_uu[1:], [dth[2]]]), dzs / ells


def autograd(x, z, r, cov, ells, sf2, noise, eps, mode, want_z=True):
    """(lml, dtheta (d + 2,), dZ or None) by torch FP64 CPU autograd of the Woodbury chain with a length-scale vector."""
    import torch
    n, q = r.shape
    m, d = z.shape
    theta = torch.tensor(np.log(np.concatenate([[sf2], np.asarray(ells, dtype=np.float64), [noise]])), dtype=torch.float64,
                         requires_grad=True)
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=bool(want_z))
    xt, rt = torch.tensor(np.asarray(x, dtype=np.float64)), torch.tensor(np.asarray(r, dtype=np.float64))
    sf, el, s2 = torch.exp(theta[0]), torch.exp(theta[1:1 + d]), torch.exp(theta[1 + d])
    xs, zs = xt / el, zt / el
    eye = torch.eye(m, dtype=torch.float64)
    lu = torch.linalg.cholesky(sg._kcov_torch(torch, zs, zs, cov, 1.0, sf) + eps * sf * eye)
    a = torch.linalg.solve_triangular(lu, sg._kcov_torch(torch, xs, zs, cov, 1.0, sf).T, upper=False).T
    qd = (a * a).sum(dim=1)
    lam = (sf - qd + s2) if mode == 0 else s2 * torch.ones(n, dtype=torch.float64)
    aw = a / lam[:, None]
    lb = torch.linalg.cholesky(eye + a.T @ aw)
    gamma = torch.linalg.solve_triangular(lb, aw.T @ rt, upper=False)
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * torch.log(lam).sum() - q * torch.log(torch.diagonal(lb)).sum()
           - 0.5 * (rt * rt / lam[:, None]).sum() + 0.5 * (gamma * gamma).sum())
    if mode == 1:
        lml = lml - 0.5 * q * (sf - qd).sum() / s2
    lml.backward()
    return float(lml.item()), theta.grad.numpy().copy(), (zt.grad.numpy().copy() if want_z else None)


def central_theta(x, z, r, cov, ells, sf2, noise, eps, mode, step=1e-5):
    """Central differences of sparse_numpy.woodbury on the scaled inputs w.r.t. theta (d + 2,)."""
    th0 = np.log(np.concatenate([[sf2], np.asarray(ells, dtype=np.float64), [noise]]))
    out = np.empty(th0.shape[0])
    for k in range(th0.shape[0]):
        vals = []
        for s in (step, -step):
            th = th0.copy()
            th[k] += s
            v = np.exp(th)
            vals.append(sn.woodbury(x / v[1:-1], z / v[1:-1], r, cov, 1.0, v[0], v[-1], eps, mode)[0])
        out[k] = (vals[0] - vals[1]) / (2 * step)
    return out


def pair_scratch_bytes(na, nb, d):
    """cimrgp_cov_pair_grad_ard_scratch_bytes by its formula: the twin's slices and tiles, 128 d + 1 + d doubles each."""
    return 8 * sg.pair_slices(na, nb)[0] * ((nb + 127) // 128) * (128 * d + 1 + d)
