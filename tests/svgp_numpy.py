"""torch FP64 CPU restatement of the variational sparse GP (include/cimrgp_svgp.h, DESIGN.md "Variational sparse GP with a
Student-t likelihood"), shared by tests/test_svgp_host.py and the GPU tests.  The objective and the latent prediction are
written twice:

  dense   q(u) = N(L_u mu, L_u S L_u^T) unwhitened, q(f) from K_fu K_uu^-1 forms with the n x n matrix
          K_fu K_uu^-1 K_uf, and KL(q(u) || N(0, K_uu)) from its definition;
  chain   the whitened chain the device runs: A = K_fu L_u^-T, W = A P^-T, m = W P^T mu, v = kdiag - sum A^2 + sum W^2,
          KL = 1/2 (|P^-1|_F^2 + mu^T mu - m + 2 sum log diag P).

K_uu is jittered the same way in both, K_uu + (eps sf + white) I.  Gradients are autograd of either form; the gap between
the two on the same inputs is the oracle's own error.  theta = (log sf, log l (1 or d), log s2, log v_1 .. log v_d -- the
last d only with a linear term); mu is (q, m), P is (q, m, m) lower triangular (its strict upper triangle is ignored).
Covariance ids are those of include/cimrgp.h; likelihoods 'gaussian' and 'student_t'."""
import math

import numpy as np
import torch

import sparse_grad_numpy as sg

H_DEFAULT = 20


def theta_of(ell, sf2, s2, lin=None):
    parts = [[sf2], np.atleast_1d(np.asarray(ell, dtype=np.float64)), [s2]]
    if lin is not None:
        parts.append(np.asarray(lin, dtype=np.float64))
    return np.log(np.concatenate(parts))


def log_lik(lik, e, s2, nu):
    """log p(y | f) at e = y - f (torch)."""
    if lik == 'gaussian':
        return -0.5 * torch.log(2 * np.pi * s2) - 0.5 * e * e / s2
    if lik != 'student_t':
        raise ValueError(lik)
    const = float(torch.lgamma(torch.tensor(0.5 * (nu + 1.0), dtype=torch.float64))
                  - torch.lgamma(torch.tensor(0.5 * nu, dtype=torch.float64)))
    return const - 0.5 * torch.log(nu * np.pi * s2) - 0.5 * (nu + 1.0) * torch.log1p(e * e / (nu * s2))


def expected_log_lik(lik, y, mean, var, s2, nu, nodes=H_DEFAULT):
    """E_i = pi^-1/2 sum_h omega_h log p(y_i | m_i + sqrt(2 v_i) x_h), elementwise over the shape of ``y``."""
    xh, wh = np.polynomial.hermite.hermgauss(nodes)
    xh, wh = torch.tensor(xh), torch.tensor(wh)
    f = mean[..., None] + torch.sqrt(2.0 * var)[..., None] * xh
    return (log_lik(lik, y[..., None] - f, s2, nu) * wh).sum(-1) / np.sqrt(np.pi)


def _unpack(theta, ne, linear):
    sf, el, s2 = torch.exp(theta[0]), torch.exp(theta[1:1 + ne]), torch.exp(theta[1 + ne])
    v = torch.exp(theta[2 + ne:]) if linear else None
    return sf, el, s2, v


def _kernel(cov, sf, el, v):
    def k(a, b):
        out = sg._kcov_torch(torch, a / el, b / el, cov, 1.0, sf)
        return out if v is None else out + (a * v) @ b.T

    def kdiag(a, white):
        out = sf + white + torch.zeros(a.shape[0], dtype=torch.float64)
        return out if v is None else out + (a * a * v).sum(dim=1)

    return k, kdiag


def moments(form, z, xq, cov, theta, mu, p, ne, linear, white, eps):
    """(mean (nq x q), var (nq x q), KL summed over the outputs) of q(f) at ``xq`` by ``form`` ('dense' or 'chain'), torch."""
    m, q = z.shape[0], mu.shape[0]
    sf, el, _, v = _unpack(theta, ne, linear)
    k, kdiag = _kernel(cov, sf, el, v)
    eye = torch.eye(m, dtype=torch.float64)
    kuu = k(z, z) + (eps * sf + white) * eye
    lu = torch.linalg.cholesky(kuu)
    kd = kdiag(xq, white)
    means, variances, kl = [], [], 0.0
    if form == 'chain':
        a = torch.linalg.solve_triangular(lu, k(xq, z).T, upper=False).T
        qd = (a * a).sum(dim=1)
        for c in range(q):
            pc = torch.tril(p[c])
            w = torch.linalg.solve_triangular(pc, a.T, upper=False).T
            means.append(w @ (pc.T @ mu[c]))
            variances.append(kd - qd + (w * w).sum(dim=1))
            pinv = torch.linalg.solve_triangular(pc, eye, upper=False)
            kl = kl + 0.5 * ((pinv * pinv).sum() + mu[c] @ mu[c] - m + 2.0 * torch.log(torch.diagonal(pc)).sum())
    elif form == 'dense':
        b = torch.linalg.solve(kuu, k(xq, z).T)                  # K_uu^-1 K_uf   (m x nq)
        qff = k(xq, z) @ b                                       # the n x n definition
        for c in range(q):
            pc = torch.tril(p[c])
            s_u = lu @ torch.linalg.inv(pc @ pc.T) @ lu.T
            m_u = lu @ mu[c]
            means.append(b.T @ m_u)
            variances.append(kd - torch.diagonal(qff) + torch.diagonal(b.T @ s_u @ b))
            kl = kl + 0.5 * (torch.trace(torch.linalg.solve(kuu, s_u)) + m_u @ torch.linalg.solve(kuu, m_u) - m
                             + torch.logdet(kuu) - torch.logdet(s_u))
    else:
        raise ValueError(form)
    return torch.stack(means, dim=1), torch.stack(variances, dim=1), kl


def _tensors(x, z, y, theta, mu, p, grad):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    th, mt, pt = t(theta), t(mu), t(p)
    for leaf in (th, mt, pt):
        leaf.requires_grad_(grad)
    return t(x), t(z), None if y is None else t(y), th, mt, pt


def elbo(form, x, z, y, cov, theta, mu, p, lik, nu=3.0, white=0.01, eps=1e-6, linear=False, nodes=H_DEFAULT, grad=True):
    """(F, dtheta, dmu, dP) -- the gradients None without ``grad`` -- with F = sum_c [sum_i E_ic - KL_c]; dP is lower
    triangular.  ``ne`` follows from the length of theta: 1 + ne + 1 (+ d) entries."""
    d = x.shape[1]
    ne = len(theta) - 2 - (d if linear else 0)
    xt, zt, yt, th, mt, pt = _tensors(x, z, y, theta, mu, p, grad)
    mean, var, kl = moments(form, zt, xt, cov, th, mt, pt, ne, linear, white, eps)
    if not bool((var > 0).all()):
        raise np.linalg.LinAlgError("a latent variance is not positive")
    f = expected_log_lik(lik, yt, mean, var, torch.exp(th[1 + ne]), nu, nodes).sum() - kl
    if not grad:
        return float(f.item()), None, None, None
    f.backward()
    return float(f.item()), th.grad.numpy().copy(), mt.grad.numpy().copy(), np.tril(pt.grad.numpy())


def predict(form, x, z, xs, cov, theta, mu, p, white=0.01, eps=1e-6, linear=False):
    """Latent (mean (ns x q), var (ns x q)) at ``xs``."""
    d = x.shape[1]
    ne = len(theta) - 2 - (d if linear else 0)
    _, zt, _, th, mt, pt = _tensors(x, z, None, theta, mu, p, False)
    mean, var, _ = moments(form, zt, torch.tensor(np.asarray(xs, dtype=np.float64)), cov, th, mt, pt, ne, linear, white, eps)
    return mean.numpy(), var.numpy()


def min_variance(x, z, cov, theta, mu, p, white=0.01, eps=1e-6, linear=False):
    d = x.shape[1]
    ne = len(theta) - 2 - (d if linear else 0)
    xt, zt, _, th, mt, pt = _tensors(x, z, None, theta, mu, p, False)
    return float(moments('chain', zt, xt, cov, th, mt, pt, ne, linear, white, eps)[1].min())


def central(x, z, y, cov, theta, mu, p, lik, step=1e-5, indices=None, **kw):
    """Central differences of the chain form's F w.r.t. (theta, mu, the lower triangle of P), packed in that order: (the
    differences at ``indices`` of the packed vector (default: all), ``pack``)."""
    q, m = mu.shape
    rows, cols = np.tril_indices(m)

    def pack(th, mm, pp):
        return np.concatenate([th, mm.ravel()] + [pp[c][rows, cols] for c in range(q)])

    def unpack(vec):
        nt = len(theta)
        th, mm = vec[:nt], vec[nt:nt + q * m].reshape(q, m)
        pp = np.zeros((q, m, m))
        rest = vec[nt + q * m:].reshape(q, -1)
        for c in range(q):
            pp[c][rows, cols] = rest[c]
        return th, mm, pp

    v0 = pack(np.asarray(theta, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(p, dtype=np.float64))
    indices = np.arange(v0.size) if indices is None else np.asarray(indices)
    out = np.empty(indices.size)
    for j, k in enumerate(indices):
        hi, lo = v0.copy(), v0.copy()
        hi[k] += step
        lo[k] -= step
        out[j] = (elbo('chain', x, z, y, cov, *unpack(hi), lik, grad=False, **kw)[0]
                  - elbo('chain', x, z, y, cov, *unpack(lo), lik, grad=False, **kw)[0]) / (2 * step)
    return out, pack


def gaussian_optimum(x, z, y, cov, theta, white=0.01, eps=1e-6, linear=False):
    """(mu, P) of the optimal q(v) under the Gaussian likelihood with variance s2: P = L_B, mu = L_B^-T gamma of the VFE fit
    with noise s2 (B = I + A^T A / s2, gamma = L_B^-1 A^T y / s2), by the chain in NumPy."""
    d = x.shape[1]
    ne = len(theta) - 2 - (d if linear else 0)
    xt, zt, yt, th, _, _ = _tensors(x, z, y, theta, np.zeros((1, 1)), np.zeros((1, 1, 1)), False)
    sf, el, s2, v = _unpack(th, ne, linear)
    k, _ = _kernel(cov, sf, el, v)
    m = z.shape[0]
    eye = torch.eye(m, dtype=torch.float64)
    lu = torch.linalg.cholesky(k(zt, zt) + (eps * sf + white) * eye)
    a = torch.linalg.solve_triangular(lu, k(xt, zt).T, upper=False).T
    lb = torch.linalg.cholesky(eye + a.T @ a / s2)
    gamma = torch.linalg.solve_triangular(lb, a.T @ yt / s2, upper=False)            # m x q
    mu = torch.linalg.solve_triangular(lb.T, gamma, upper=True)
    q = y.shape[1]
    return mu.T.numpy().copy(), np.repeat(lb.numpy()[None], q, axis=0)


def problem(n, m, d, q, seed, outliers=False):
    """A smooth regression problem on [-1, 1]^d: (x (n x d), z (m x d, rows of x), y (n x q))."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n, d))
    z = x[rng.choice(n, size=m, replace=False)].copy()
    f = np.stack([np.sin(3.0 * x[:, 0] + c) + 0.5 * x[:, -1] * (c + 1) for c in range(q)], axis=1)
    y = f + 0.1 * rng.normal(size=(n, q))
    if outliers:
        y[::17] += 3.0
    return x, z, y


def perturbed_posterior(m, q, seed):
    """A (mu, P) away from any optimum: mu ~ 0.5 N(0, 1), P = chol of a well-conditioned SPD matrix."""
    rng = np.random.default_rng(seed)
    mu = 0.5 * rng.normal(size=(q, m))
    p = np.empty((q, m, m))
    for c in range(q):
        g = rng.normal(size=(m, m)) / np.sqrt(m)
        p[c] = np.linalg.cholesky(2.0 * np.eye(m) + g @ g.T)
    return mu, p


# ---- cimrgp_svgp_rows in NumPy, in any float type ------------------------------------------------------------------------
def quadrature(lik, y, mean, var, s2, nu, ft, nodes=H_DEFAULT):
    """The four Gauss-Hermite sums of one column at the given latent moments, evaluated in the float type ``ft``:
    ({E, g1, g2, gs}, the sums of the magnitudes of their terms), each (n,).  The nodes are numpy.polynomial's FP64 values."""
    xh, wh = np.polynomial.hermite.hermgauss(nodes)
    xh, wh = xh.astype(ft), wh.astype(ft)
    y, mean, var, s2, nu = (np.asarray(a, dtype=ft) for a in (y, mean, var, s2, nu))
    pi = ft(np.pi) + ft(1.2246467991473532e-16)           # pi beyond FP64 where ``ft`` holds it
    c = ft(1) / np.sqrt(pi)
    root = np.sqrt(ft(2) * var)
    e = y[:, None] - (mean[:, None] + root[:, None] * xh)
    if lik == 'gaussian':
        lp = -ft(0.5) * np.log(ft(2) * pi * s2) - ft(0.5) * e * e / s2
        df, ds = e / s2, ft(0.5) * e * e / s2 - ft(0.5)
    else:
        const = ft(math.lgamma(0.5 * (float(nu) + 1.0)) - math.lgamma(0.5 * float(nu)))
        lp = const - ft(0.5) * np.log(nu * pi * s2) - ft(0.5) * (nu + ft(1)) * np.log1p(e * e / (nu * s2))
        df = (nu + ft(1)) * e / (nu * s2 + e * e)
        ds = ft(0.5) * (nu + ft(1)) * e * e / (nu * s2 + e * e) - ft(0.5)
    terms = dict(E=wh * lp, g1=wh * df, g2=wh * df * xh / root[:, None], gs=wh * ds)
    return {k: c * t.sum(axis=1) for k, t in terms.items()}, {k: c * np.abs(t).sum(axis=1) for k, t in terms.items()}


def row_moments(a, w, gamma, kdiag, ft):
    """(m_i, v_i, sum_j |W_ij gamma_j|, kdiag_i + sum A^2 + sum W^2) of the rows in ``ft``."""
    a, w, gamma, kdiag = (np.asarray(t, dtype=ft) for t in (a, w, gamma, kdiag))
    sa, sw = (a * a).sum(axis=1), (w * w).sum(axis=1)
    return (w * gamma).sum(axis=1), kdiag - sa + sw, (np.abs(w) * np.abs(gamma)).sum(axis=1), np.abs(kdiag) + sa + sw


# ---- the plugin's fit on the CPU -----------------------------------------------------------------------------------------
def fit_predict(x, y, xs, lik, num_inducing, max_iters, seed=0, nu=3.0, white=0.01, eps=1e-6):
    """SVIGP_RBF's fit (RBF, ARD + linear, Z drawn by its rule, the same start and the same L-BFGS-B driver) with this
    module's chain form and autograd in place of the device, and the latent mean at ``xs`` in the units of ``y``."""
    from cimrgp_amd import Hyper
    xm, xsd, ym, ysd = x.mean(0), x.std(0), y.mean(0), y.std(0)
    xn, yn = (x - xm) / xsd, (y - ym) / ysd
    d = x.shape[1]
    z = xn[np.random.RandomState(seed).permutation(x.shape[0])[:num_inducing]]
    theta = theta_of(np.ones(d), 1.0, 0.01, np.ones(d))
    kw = dict(nu=nu, white=white, eps=eps, linear=True)
    mu, p = gaussian_optimum(xn, z, yn, 0, theta, white=white, eps=eps, linear=True)
    res, theta, mu, p = Hyper.maximize_elbo(lambda t, m_, p_: elbo('chain', xn, z, yn, 0, t, m_, p_, lik, **kw), theta, mu, p, max_iters)
    mean, _ = predict('chain', xn, z, (xs - xm) / xsd, 0, theta, mu, p, white=white, eps=eps, linear=True)
    return mean * ysd + ym, theta, -res.fun
