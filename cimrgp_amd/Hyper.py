"""Hyper-parameter learning on the host: the rules every plugin and the model share ("Hyper-parameter learning on
the host").  One place each for the ARD input scaling, the optimisers' parameter vector [log sf, log l .., log noise, (log v ..), (Z)],
the L-BFGS-B call with its score of a failed trial point, and the sum of a layer's per-block objectives with its failure
codes; and for the variational sparse GP the vector's further part [mu.ravel(), vech(P) per output] with its driver
(:func:`pack_posterior`, :func:`maximize_elbo`).  Host only: nothing here calls the library."""
import numpy as np
import torch

from . import device as dev

#: what a trial point scores (with a zero gradient) when its covariance is not positive definite
FAILED_SCORE = 1e100


def unit_lengthscale(x, lengthscales):
    """``(scale, x * scale)``: ``scale`` = 1 / lengthscales (float64 on the host, then cast to ``x``'s dtype on its device);
    the scaled inputs are what every kernel takes, at unit length-scale, under ARD."""
    scale = torch.as_tensor(1.0 / np.asarray(lengthscales, dtype=np.float64), dtype=x.dtype, device=x.device)
    return scale, scaled(x, scale)


def scaled(x, scale):
    """Inputs ``x`` (test inputs, say) in the units of an existing ``scale`` of :func:`unit_lengthscale`."""
    return (x * scale).contiguous()


def pack_theta(sf, ell, noise):
    """[log sf, log l (one per entry of ``ell``), log noise]."""
    return np.log([sf] + list(np.atleast_1d(ell)) + [noise])


def unpack_theta(theta, n_ell=None):
    """``(ell, sf, noise)`` of a parameter vector; what follows them (Z) is left alone.  ``n_ell`` None: one isotropic
    length-scale, a float; else ARD with ``n_ell`` length-scales, a fresh (n_ell,) array."""
    vals = np.exp(theta[:(1 if n_ell is None else n_ell) + 2])
    return (float(vals[1]) if n_ell is None else vals[1:-1].copy()), float(vals[0]), float(vals[-1])


def append_linear(theta, linear):
    """``theta`` = [log sf, log l .., log noise] with the d log-variances of a linear term appended: [.., log v_1 .. log v_d];
    Z, where it is learned, follows them."""
    return np.concatenate([np.asarray(theta, dtype=np.float64), np.log(np.asarray(linear, dtype=np.float64).reshape(-1))])


def split_linear(theta, n_linear, n_ell=None):
    """``(head, linear, rest)`` of a parameter vector laid out by :func:`append_linear`: the [log sf, log l .., log noise] that
    :func:`unpack_theta` reads, the ``n_linear`` variances (a fresh array, not their logarithms) and what follows them (Z)."""
    nt = (1 if n_ell is None else n_ell) + 2
    return theta[:nt], np.exp(theta[nt:nt + n_linear]), theta[nt + n_linear:]


def minimize_lml(objective, theta0, max_iters, jac=True):
    """L-BFGS-B (SciPy) maximising ``objective(theta)`` -> ``(lml, grad)``, or ``lml`` alone with ``jac=None`` (SciPy's
    two-point differences).  An objective that raises ``numpy.linalg.LinAlgError`` or returns None marks a failed trial
    point, which scores FAILED_SCORE with a zero gradient.  Returns SciPy's result (of the NEGATED objective)."""
    from scipy.optimize import minimize

    def negated(theta):
        try:
            value = objective(theta)
        except np.linalg.LinAlgError:
            value = None
        if value is None:
            return (FAILED_SCORE, np.zeros(theta.shape[0])) if jac else FAILED_SCORE
        if not jac:
            return -value
        lml, grad = value
        return -lml, -grad

    return minimize(negated, theta0, jac=jac, method='L-BFGS-B', options=dict(maxiter=max_iters))


def pack_posterior(mu, p):
    """The variational part of the parameter vector [log sf, log l .., log s2, (log v ..), mu.ravel(), vech(P_0), vech(P_1) ..]
    of the variational sparse GP (``SVGP.SVGPBlock``): ``mu`` (q, m), then per output the lower triangle of ``p[c]`` (m x m)
    row by row, its diagonal as logarithms, which keeps it positive."""
    mu, p = np.asarray(mu, dtype=np.float64), np.asarray(p, dtype=np.float64)
    rows, cols = np.tril_indices(p.shape[1])
    parts = [mu.ravel()]
    for pc in p:
        v = pc[rows, cols].copy()
        v[rows == cols] = np.log(v[rows == cols])
        parts.append(v)
    return np.concatenate(parts)


def unpack_posterior(vec, q, m):
    """``(mu (q, m), P (q, m, m) lower triangular)`` of a vector laid out by :func:`pack_posterior`."""
    vec = np.asarray(vec, dtype=np.float64)
    rows, cols = np.tril_indices(m)
    mu = vec[:q * m].reshape(q, m).copy()
    tri = vec[q * m:].reshape(q, rows.shape[0])
    p = np.zeros((q, m, m))
    for c in range(q):
        v = tri[c].copy()
        v[rows == cols] = np.exp(v[rows == cols])
        p[c][rows, cols] = v
    return mu, p


def posterior_gradient(dmu, dp, p):
    """The gradient w.r.t. :func:`pack_posterior`'s vector from dF/dmu (q, m), dF/dP (q, m, m) and P: the diagonal's
    entries are w.r.t. log P_ii, P_ii dF/dP_ii."""
    dmu, dp, p = (np.asarray(a, dtype=np.float64) for a in (dmu, dp, p))
    rows, cols = np.tril_indices(p.shape[1])
    parts = [dmu.ravel()]
    for gc, pc in zip(dp, p):
        v = gc[rows, cols].copy()
        v[rows == cols] *= np.diagonal(pc)
        parts.append(v)
    return np.concatenate(parts)


def maximize_elbo(elbo_grad, theta0, mu0, p0, max_iters):
    """L-BFGS-B over the whole vector [theta, mu.ravel(), vech(P) per output] on the analytic gradient: ``elbo_grad(theta,
    mu, P)`` -> ``(F, dtheta, dmu, dP)`` in NumPy.  A trial point that raises LinAlgError scores as :func:`minimize_lml` has
    it.  Returns (SciPy's result of the negated objective, theta, mu, P) at the optimum."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    nt = theta0.shape[0]
    q, m = np.shape(mu0)

    def objective(vec):
        mu, p = unpack_posterior(vec[nt:], q, m)
        f, dtheta, dmu, dp = elbo_grad(vec[:nt], mu, p)
        return f, np.concatenate([dtheta, posterior_gradient(dmu, dp, p)])

    res = minimize_lml(objective, np.concatenate([theta0, pack_posterior(mu0, p0)]), max_iters)
    mu, p = unpack_posterior(res.x[nt:], q, m)
    return res, res.x[:nt].copy(), mu, p


def sum_block_objectives(regions, evaluate, n_grad=3):
    """``(lml, grad, failure)``: the sums of ``evaluate(l)`` -> ``(lml, grad)`` over ``regions``, in their order; grad has the
    length of the first block's gradient -- 3, or d + 2 under ARD -- and ``n_grad`` zeros when no block gave one.  A
    block that raises ``numpy.linalg.LinAlgError`` is left out of the sums and raises failure to 1, one that raises the
    'schedule watchdog' RuntimeError to ``device.INFO_WATCHDOG``; any other exception propagates.  failure is the largest
    code met: 0 = every block is fine."""
    lml, grad, failure = 0.0, None, 0.0
    for l in regions:
        try:
            a, g = evaluate(l)
        except np.linalg.LinAlgError:
            failure = max(failure, 1.0)
            continue
        except RuntimeError as e:
            if 'schedule watchdog' not in str(e):
                raise
            failure = max(failure, float(dev.INFO_WATCHDOG))
            continue
        if grad is None:
            grad = np.zeros(np.shape(g))
        lml, grad = lml + a, grad + g
    return lml, (np.zeros(n_grad) if grad is None else grad), failure
