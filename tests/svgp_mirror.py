"""The device's analytic gradient of the variational sparse GP (cimrgp_amd/SVGP.py) replayed on the CPU in torch FP64: the
row quantities g1, g2 and the n x m steps in plain torch, the m x m algebra by SVGP's OWN ``column_terms`` and
``kuu_weight``, and the pair contractions as autograd of sum G o K(theta) with the weights G held fixed.  What it returns is
compared with autograd of the objective itself (tests/svgp_numpy.py), which shares none of these steps."""
import numpy as np
import torch

import svgp_numpy as so
from cimrgp_amd import SVGP


def row_terms(lik, y, mean, var, s2, nu, nodes=so.H_DEFAULT):
    """(E, g1 = dE/dm, g2 = dE/dv, dE/dlog s2) per row by the closed derivatives of the quadrature sum (torch, no autograd)."""
    xh, wh = np.polynomial.hermite.hermgauss(nodes)
    xh, wh = torch.tensor(xh), torch.tensor(wh)
    root = torch.sqrt(2.0 * var)
    e = y[:, None] - (mean[:, None] + root[:, None] * xh)
    if lik == 'gaussian':
        df, ds = e / s2, 0.5 * e * e / s2 - 0.5
    else:
        df, ds = (nu + 1.0) * e / (nu * s2 + e * e), 0.5 * (nu + 1.0) * e * e / (nu * s2 + e * e) - 0.5
    lp = so.log_lik(lik, e, torch.as_tensor(s2, dtype=torch.float64), nu)
    c = 1.0 / np.sqrt(np.pi)
    return c * (lp * wh).sum(1), c * (df * wh).sum(1), c * (df * wh * xh).sum(1) / root, c * (ds * wh).sum(1)


def elbo_grad(x, z, y, cov, theta, mu, p, lik, nu=3.0, white=0.01, eps=1e-6, linear=False):
    """(F, dtheta, dmu, dP) by the device's chain rule on the CPU."""
    d = x.shape[1]
    ne = len(theta) - 2 - (d if linear else 0)
    xt, zt, yt, th, mt, pt = so._tensors(x, z, y, theta, mu, p, False)
    th.requires_grad_(True)
    sf, el, s2, v = so._unpack(th, ne, linear)
    k, kdiag = so._kernel(cov, sf, el, v)
    m, q = z.shape[0], mu.shape[0]
    eye = torch.eye(m, dtype=torch.float64)
    kuu, kfu, kd = k(zt, zt) + (eps * sf + white) * eye, k(xt, zt), kdiag(xt, white)
    with torch.no_grad():
        lu = torch.linalg.cholesky(kuu)
        a = torch.linalg.solve_triangular(lu, kfu.T, upper=False).T
        abar, ata, t = torch.zeros_like(a), torch.zeros(m, m, dtype=torch.float64), torch.zeros(x.shape[0], dtype=torch.float64)
        f, ds2 = 0.0, 0.0
        dmu, dp = torch.empty_like(mt), torch.empty_like(pt)
        for c in range(q):
            pc = torch.tril(pt[c])
            w = torch.linalg.solve_triangular(pc, a.T, upper=False).T
            mean, var = w @ (pc.T @ mt[c]), kd - (a * a).sum(1) + (w * w).sum(1)
            e_i, g1, g2, gs = row_terms(lik, yt[:, c], mean, var, float(s2), nu)
            dmu[c], dp[c], ata_c, kl = SVGP.column_terms(pc, mt[c], a.T @ (g2[:, None] * a), a.T @ g1)
            yc = torch.linalg.solve_triangular(pc.T, w.T, upper=True).T
            abar += torch.outer(g1, mt[c]) + 2.0 * g2[:, None] * (yc - a)
            ata, t, f, ds2 = ata + ata_c, t + g2, f + e_i.sum() - kl, ds2 + gs.sum()
        gfu = torch.linalg.solve_triangular(lu.T, abar.T, upper=True).T          # Abar L_u^-1
        guu = SVGP.kuu_weight(lu, ata)
    ((gfu * kfu).sum() + (guu * kuu).sum() + (t * kd).sum()).backward()
    dtheta = th.grad.numpy().copy()
    dtheta[1 + ne] += float(ds2)
    return float(f), dtheta, dmu.numpy(), dp.numpy()
