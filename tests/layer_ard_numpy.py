"""NumPy / SciPy restatements for the ARD layers of the multiresolution model (include/cimrgp_layer_ard.h, DESIGN.md "ARD
length-scales for the model's layers"), shared by tests/test_layer_ard_host.py and the GPU tests: the four covariances
with one length-scale per input dimension and d k / d log l_k, a block's log marginal likelihood with its d + 2
gradient entries, the dense residual chain and the L-BFGS-B driver over theta = (log sf, log l_1 .. log l_d, log noise).
A scalar length-scale is the isotropic covariance; its gradient then has 3 entries."""
import numpy as np
import scipy.linalg as sla

COVS = {0: None, 1: 0.5, 2: 1.5, 3: 2.5}        # CIMRGP_COV_* -> Matern nu (None: RBF)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def cov_ard(xa, xb, cov, ells, sf2, want_grad=True):
    """(k, [d k / d log l_k for every k]) of every pair under length-scales ``ells`` (d,), or a scalar for all dimensions
    (then one derivative, w.r.t. the common log l).  With u = x / l and r = |u - u'|: d k / d log l_k = D(r) du_k^2 / r^2,
    D = -r dk/dr the isotropic derivative; 0 at r = 0 (for Matern 1/2 by convention, as the device takes it)."""
    iso = np.ndim(ells) == 0
    ells = np.full(xa.shape[1], float(ells)) if iso else np.asarray(ells, dtype=np.float64)
    du2 = ((xa[:, None, :] - xb[None, :, :]) / ells) ** 2
    d2 = du2.sum(-1)
    nu = COVS[cov]
    if nu is None:
        k = sf2 * np.exp(-0.5 * d2)
        w = k                                   # D / r^2
    else:
        t = np.sqrt(2 * nu) * np.sqrt(d2)
        v = np.exp(-t)
        if nu == 0.5:
            k, big_d = sf2 * v, sf2 * t * v
        elif nu == 1.5:
            k, big_d = sf2 * (1 + t) * v, sf2 * t * t * v
        else:
            k, big_d = sf2 * (1 + t + t * t / 3) * v, sf2 * t * t * (1 + t) * v / 3
        w = np.where(d2 > 0, big_d / np.where(d2 > 0, d2, 1.0), 0.0)
    if not want_grad:
        return k, None
    if iso:
        return k, [w * d2]
    return k, [w * du2[:, :, e] for e in range(xa.shape[1])]


def lml_grad(x, r, cov, ells, sf2, noise):
    """LML of targets r (n x q) and its gradient w.r.t. (log sf2, log l_1 .. log l_d, log noise), (d + 2,); a scalar
    ``ells``: (log sf2, log l, log noise)."""
    n, q = r.shape
    k, dks = cov_ard(x, x, cov, ells, sf2)
    chol = sla.cholesky(k + noise * np.eye(n), lower=True)
    alpha = sla.cho_solve((chol, True), r)
    lml = -0.5 * np.sum(r * alpha) - q * np.sum(np.log(np.diag(chol))) - 0.5 * n * q * np.log(2 * np.pi)
    g = alpha @ alpha.T - q * sla.cho_solve((chol, True), np.eye(n))
    return lml, np.array([0.5 * np.sum(g * k)] + [0.5 * np.sum(g * dk) for dk in dks] + [0.5 * noise * np.trace(g)])


class Sparse(object):
    """What makes a layer sparse: m = num_inducing (stride rule), mode 0 FITC / 1 VFE, eps = jitter."""

    def __init__(self, m, mode=0, eps=1e-6):
        self.m, self.mode, self.eps = int(m), int(mode), float(eps)


def inducing_rows(n, m):
    """SparseKernel's 'stride' rule: rows floor((k + 0.5) n / m), k = 0 .. m - 1, m = min(n, num_inducing)."""
    m = min(n, m)
    return ((2 * np.arange(m, dtype=np.int64) + 1) * n) // (2 * m)


def _vector(ells, d):
    return np.full(d, float(ells)) if np.ndim(ells) == 0 else np.asarray(ells, dtype=np.float64)


def fit_predict(xn, y, bounds, layers, xsn=None, tbounds=None):
    """The residual chain with per-region bias: layers = [(cov, ells, sf2, noise)] for an exact layer, (cov, ells, sf2,
    noise, Sparse) for an inducing-point one (sparse_numpy.woodbury on x / l and Z / l at unit length-scale).  Returns
    (f_bar after the last layer, [f_bar BEFORE each layer], mean, var) -- mean and var (noise of the last layer included)
    at the test points ``xsn`` under ``tbounds`` when given, else None."""
    import sparse_numpy as sn
    f_bar, before = np.zeros_like(y), []
    mean = var = None
    if xsn is not None:
        mean, var = np.zeros((xsn.shape[0], y.shape[1])), np.zeros(xsn.shape[0])
    for j, layer in enumerate(layers):
        cov, ells, sf2, noise = layer[:4]
        sp = layer[4] if len(layer) > 4 else None
        before.append(f_bar)
        mu = np.zeros_like(y)
        for l, (a, b) in enumerate(bounds[j]):
            r = y[a:b] - f_bar[a:b]
            bias = r.mean(axis=0)
            ta, tb = tbounds[j][l] if xsn is not None else (0, 0)
            last = noise if j == len(layers) - 1 else 0.0
            if sp is not None:
                s = 1.0 / _vector(ells, xn.shape[1])
                xa = xn[a:b] * s
                z = xa[inducing_rows(b - a, sp.m)]
                at = xa if xsn is None else np.vstack([xa, xsn[ta:tb] * s])
                _, m_at, v_at = sn.woodbury(xa, z, r - bias, cov, 1.0, sf2, noise, sp.eps, sp.mode, at)
                mu[a:b] = m_at[:b - a] + bias
                if xsn is not None:
                    mean[ta:tb] += m_at[b - a:] + bias
                    var[ta:tb] += v_at[b - a:] + last
                continue
            k, _ = cov_ard(xn[a:b], xn[a:b], cov, ells, sf2, want_grad=False)
            chol = sla.cholesky(k + noise * np.eye(b - a), lower=True)
            alpha = sla.cho_solve((chol, True), r - bias)
            mu[a:b] = r - noise * alpha
            if xsn is not None:
                ks, _ = cov_ard(xsn[ta:tb], xn[a:b], cov, ells, sf2, want_grad=False)
                mean[ta:tb] += ks @ alpha + bias
                w = sla.solve_triangular(chol, ks.T, lower=True)
                var[ta:tb] += sf2 - np.sum(w * w, axis=0) + last
        f_bar = f_bar + mu
    return f_bar, before, mean, var


def layer_objective(xn, r, bounds_j, cov, ells, sf2, noise, sparse=None):
    """Sum over the regions of one layer of the objective on the residual targets ``r`` (N x q) with per-region bias:
    :func:`lml_grad` for an exact layer, sparse_ard_numpy.chain for a :class:`Sparse` one (a scalar ``ells``: the d
    length-scale entries of its gradient added up)."""
    import sparse_ard_numpy as sa
    lml, grad = 0.0, 0.0
    for a, b in bounds_j:
        rc = r[a:b] - r[a:b].mean(axis=0)
        if sparse is None:
            v, g = lml_grad(xn[a:b], rc, cov, ells, sf2, noise)
        else:
            z = xn[a:b][inducing_rows(b - a, sparse.m)]
            v, g, _ = sa.chain(xn[a:b], z, rc, cov, _vector(ells, xn.shape[1]), sf2, noise, sparse.eps, sparse.mode)
            if np.ndim(ells) == 0:
                g = np.array([g[0], g[1:-1].sum(), g[-1]])
        lml, grad = lml + v, grad + g
    return lml, grad


def learn(xn, y, bounds, starts, max_iters=1000):
    """The NumPy driver: per layer, coarse to fine, L-BFGS-B on -sum_l LML_l of the residual targets (per-region bias) over
    theta = (log sf, log l .., log noise), then the layer fitted with the learned values.  starts = [(cov, l0, sf0)] or
    [(cov, l0, sf0, Sparse)] of the constructor's kernels, l0 a scalar (isotropic, 3 parameters) or a (d,) vector (ARD,
    d + 2).  Returns (layers, results)."""
    from scipy.optimize import minimize
    layers, results = [], []
    for j, start in enumerate(starts):
        cov, l0, sf0 = start[:3]
        sp = start[3] if len(start) > 3 else None
        f_bar = fit_predict(xn, y, bounds, layers)[0] if layers else np.zeros_like(y)
        iso = np.ndim(l0) == 0

        def objective(theta):
            v = np.exp(theta)
            try:
                lml, grad = layer_objective(xn, y - f_bar, bounds[j], cov, float(v[1]) if iso else v[1:-1], v[0], v[-1], sp)
            except np.linalg.LinAlgError:
                return 1e100, np.zeros(theta.shape[0])
            return -lml, -grad

        theta0 = np.log([sf0] + list(np.atleast_1d(l0)) + [0.01 * sf0])
        res = minimize(objective, theta0, jac=True, method='L-BFGS-B', options=dict(maxiter=max_iters))
        v = np.exp(res.x)
        layers.append((cov, float(v[1]) if iso else v[1:-1].copy(), float(v[0]), float(v[-1])) + (() if sp is None else (sp,)))
        results.append(res)
    return layers, results
