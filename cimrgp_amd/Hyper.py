"""Hyper-parameter learning on the host: the rules every plugin and the model share ("Hyper-parameter learning on
the host").  One place each for the ARD input scaling, the optimisers' parameter vector [log sf, log l .., log noise, (log v ..), (Z)],
the L-BFGS-B call with its score of a failed trial point, and the sum of a layer's per-block objectives with its failure
codes.  Host only: nothing here calls the library."""
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
