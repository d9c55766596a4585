"""The gradient of the sparse objective (include/cimrgp_sparse_grad.h, DESIGN.md "Gradients of the sparse objective") in
two independent forms, shared by tests/test_sparse_grad_host.py and the GPU tests: the NumPy chain the device runs, and
torch FP64 CPU autograd of the Woodbury chain.  Covariance ids are those of include/cimrgp.h; mode 0 = FITC, 1 = VFE.
theta = (log sf, log l, log noise)."""
import numpy as np
import scipy.linalg as sla

from grad_numpy import NU, g_of, kcov


def dk_dlogl(xa, xb, cov, ell, sf2):
    """(dk / dlog l)(xa_i, xb_j) = -r dk/dr."""
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    return g_of(xa, xb, cov, ell, sf2) * d2


def pair_grad(xa, xb, g, cov, ell, sf2, scale=1.0):
    """The contraction of cimrgp_cov_pair_grad: ((sum G o K, sum G o dK/dlog l), db (nb x d)) and the sums of magnitudes
    of the same terms, ((sum |G K|, sum |G dK|), sum_i |scale G_ij g_ij (xa_ie - xb_je)|), which scale the error bound."""
    k = kcov(xa, xb, cov, ell, sf2)
    dl = dk_dlogl(xa, xb, cov, ell, sf2)
    gg = g * g_of(xa, xb, cov, ell, sf2)
    d = xa.shape[1]
    db, mag = np.empty((xb.shape[0], d)), np.empty((xb.shape[0], d))
    for e in range(d):
        term = scale * gg * (xa[:, None, e] - xb[None, :, e])
        db[:, e] = term.sum(axis=0)
        mag[:, e] = np.abs(term).sum(axis=0)
    return (np.array([(g * k).sum(), (g * dl).sum()]), db), (np.array([np.abs(g * k).sum(), np.abs(g * dl).sum()]), mag)


def rows(v, gamma, r, w, mode, noise):
    """cimrgp_sparse_grad_rows: (beta, t, h)."""
    q = r.shape[1]
    beta = w[:, None] * (r - v @ gamma)
    h = 0.5 * ((beta * beta).sum(axis=1) - q * (w - w * w * (v * v).sum(axis=1)))
    t = h if mode == 0 else np.full(v.shape[0], -0.5 * q / noise)
    return beta, t, h


def combine(a, y, beta, b, w, t):
    """cimrgp_sparse_grad_combine."""
    return beta @ b.T - beta.shape[1] * w[:, None] * y - 2 * t[:, None] * a


def chain(x, z, r, cov, ell, sf2, noise, eps, mode):
    """(lml, dtheta (3,), dZ (m x d), parts) by the chain of DESIGN.md; parts holds M, t, the pairwise and the closed form
    of dF / dlog sf."""
    n, q = r.shape
    m = z.shape[0]
    kuu = kcov(z, z, cov, ell, sf2) + eps * sf2 * np.eye(m)
    kfu = kcov(x, z, cov, ell, sf2)
    lu = np.linalg.cholesky(kuu)
    a = sla.solve_triangular(lu, kfu.T, lower=True).T
    qd = (a * a).sum(axis=1)
    lam = (sf2 - qd + noise) if mode == 0 else np.full(n, float(noise))
    if not (lam > 0).all():
        raise np.linalg.LinAlgError("lambda not positive")
    w = 1.0 / lam
    bmat = np.eye(m) + a.T @ (a * w[:, None])
    lb = np.linalg.cholesky(bmat)
    gamma = sla.solve_triangular(lb, a.T @ (r * w[:, None]), lower=True)
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * np.log(lam).sum() - q * np.log(np.diag(lb)).sum()
           - 0.5 * (r * r * w[:, None]).sum() + 0.5 * (gamma * gamma).sum())
    if mode == 1:
        lml -= 0.5 * q * (sf2 - qd).sum() / noise
    v = sla.solve_triangular(lb, a.T, lower=True).T                      # A L_B^-T
    b = sla.solve_triangular(lb.T, gamma, lower=False)                    # L_B^-T gamma
    beta, t, h = rows(v, gamma, r, w, mode, noise)
    y = sla.solve_triangular(lb.T, v.T, lower=False).T                    # V L_B^-1 = A B^-1
    ga = combine(a, y, beta, b, w, t)
    gfu = sla.solve_triangular(lu.T, ga.T, lower=False).T                 # G_A L_u^-1
    binv = sla.cho_solve((lb, True), np.eye(m))
    if mode == 0:
        ata = a.T @ (a * t[:, None])
    else:
        ata = -0.5 * q * (bmat - np.eye(m))
    mm = b @ b.T - q * (np.eye(m) - binv) - 2 * ata
    guu = -0.5 * sla.solve_triangular(lu.T, sla.solve_triangular(lu.T, mm, lower=False).T, lower=False)
    guu = 0.5 * (guu + guu.T)
    (s_fu, dz_fu), _ = pair_grad(x, z, gfu, cov, ell, sf2)
    (s_uu, dz_uu), _ = pair_grad(z, z, guu, cov, ell, sf2, scale=2.0)     # G_uu symmetric: -2 sum_b G_jb g (z_j - z_b)
    pairwise = s_fu[0] + s_uu[0] + eps * sf2 * np.trace(guu) + sf2 * t.sum()
    closed = 0.5 * np.trace(mm) + sf2 * t.sum()
    dnoise = noise * (h.sum() + (0.5 * q / noise ** 2 * (sf2 - qd).sum() if mode == 1 else 0.0))
    dtheta = np.array([closed, s_fu[1] + s_uu[1], dnoise])
    return lml, dtheta, dz_fu + dz_uu, dict(M=mm, t=t, pairwise=pairwise, closed=closed, ga=ga, a=a)


def _kcov_torch(torch, xa, xb, cov, ell, sf2):
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    if cov == 0:
        return sf2 * torch.exp(-0.5 * d2 / ell ** 2)
    # a safe square root: the r = 0 pairs contribute the value at r = 0 and a zero derivative
    zero = d2 <= 0
    rr = torch.sqrt(torch.where(zero, torch.ones_like(d2), d2))
    rr = torch.where(zero, torch.zeros_like(d2), rr)
    t = np.sqrt(2 * NU[cov]) * rr / ell
    poly = {1: 1.0, 2: 1 + t, 3: 1 + t + t * t / 3}[cov]
    return sf2 * poly * torch.exp(-t)


def autograd(x, z, r, cov, ell, sf2, noise, eps, mode, want_z=True):
    """(lml, dtheta (3,), dZ or None) by torch FP64 CPU autograd of the restated Woodbury chain."""
    import torch
    n, q = r.shape
    m = z.shape[0]
    theta = torch.tensor(np.log([sf2, ell, noise]), dtype=torch.float64, requires_grad=True)
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=bool(want_z))
    xt, rt = torch.tensor(np.asarray(x, dtype=np.float64)), torch.tensor(np.asarray(r, dtype=np.float64))
    sf, el, s2 = torch.exp(theta[0]), torch.exp(theta[1]), torch.exp(theta[2])
    eye = torch.eye(m, dtype=torch.float64)
    lu = torch.linalg.cholesky(_kcov_torch(torch, zt, zt, cov, el, sf) + eps * sf * eye)
    a = torch.linalg.solve_triangular(lu, _kcov_torch(torch, xt, zt, cov, el, sf).T, upper=False).T
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


def central_theta(x, z, r, cov, ell, sf2, noise, eps, mode, step=1e-5):
    """Central differences of sparse_numpy.woodbury w.r.t. theta."""
    import sparse_numpy as sn
    th0 = np.log([sf2, ell, noise])
    out = np.empty(3)
    for k in range(3):
        vals = []
        for s in (step, -step):
            th = th0.copy()
            th[k] += s
            sf, el, s2 = np.exp(th)
            vals.append(sn.woodbury(x, z, r, cov, el, sf, s2, eps, mode)[0])
        out[k] = (vals[0] - vals[1]) / (2 * step)
    return out


def problem(n, m, d, seed, q=2, shift=0.05):
    """The inputs of the issue's check: x uniform on [-2, 2]^d, Z a random subset of X moved off the data by
    shift N(0, 1)."""
    import sparse_numpy as sn
    x, z, r, _ = sn.problem(n, m, d, seed, q=q)
    rng = np.random.default_rng(seed + 1000)
    return x, z + shift * rng.normal(size=z.shape), r


def pair_slices(na, nb):
    """(S, slice length) of cimrgp_cov_pair_grad by its rule: tiles x S <= 1024, a slice of at least 256 rows, a multiple
    of 8."""
    tiles = (nb + 127) // 128
    s = max(1, min(1024 // tiles, (na + 255) // 256))
    length = ((na + s - 1) // s + 7) // 8 * 8
    return (na + length - 1) // length, length


def pair_scratch_bytes(na, nb, d):
    """cimrgp_cov_pair_grad_scratch_bytes by its formula."""
    return 8 * pair_slices(na, nb)[0] * ((nb + 127) // 128) * (128 * d + 2)
