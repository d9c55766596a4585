"""Greedy inducing-point selection ("Greedy inducing-point selection").

The greedy rule picks, m times, the training row with the largest conditional variance given the rows already picked (Burt,
Rasmussen & van der Wilk 2019 / 2020; gpflow's ``ConditionalVariance`` initialiser).  That is a pivoted Cholesky
factorisation of K(X, X) stopped after m columns, and it is run matrix-free on the device (cimrgp_pivoted_cholesky,
include/cimrgp_inducing.h): n m^2 / 2 multiply-adds over an n x m factor, K never formed.  Its by-product, the residual trace
after j pivots, is tr(K - Q_j), the slack term of the VFE bound: whether m is large enough is known before any fit.

:func:`greedy_rows` works on device tensors and is what ``KernelClass.SparseKernel(inducing='greedy')`` runs per region;
:func:`select_inducing` works on host arrays and gives the ``Z=`` of every inducing-point plugin::

    Z, rows, trace = select_inducing(X, 1000, lengthscale=0.5)
    gp = SGP_FITC(Z=Z, lengthscale=0.5)

It does not learn Z: the rows are a function of the inputs and the covariance alone."""
import numpy as np
import torch

from . import device as dev
from . import device_inducing as devi
from .KernelClass import DenseMaternKernel, RBFKernel
from .RegressionInput import lengthscale_argument, non_negative, per_dimension, positive_scalar
from .Sparse import BlockCovariance


class GreedyRows(object):
    """What :func:`greedy_rows` leaves on the device: ``rows`` (int64, m), ``trace`` (float64, m + 1: trace[j] =
    tr(K - Q_j)), ``rank`` (int64, 1: the steps whose pivot residual exceeded the floor), ``diag`` (float64, n: the residual
    of the rows not picked, -1 for the picked) and ``factor`` (m x ld, ld >= n: row j is column j of L)."""

    def __init__(self, n, rows, factor, diag, trace, rank):
        self.n, self.m = int(n), int(rows.shape[0])
        self.rows, self.factor, self.diag, self.trace, self.rank = rows, factor, diag, trace, rank

    def rows_numpy(self):
        """``rows`` on the host (one read-back)."""
        return self.rows.cpu().numpy()

    def trace_numpy(self):
        """``trace`` on the host (one read-back)."""
        return self.trace.cpu().numpy()

    def rows_for(self, tol):
        """The smallest m' with trace[m'] <= tol * trace[0] (one read-back); ``m`` if no prefix reaches it."""
        tol = non_negative(tol, 'tol', finite=True)
        t = self.trace_numpy()
        hit = np.nonzero(t <= tol * t[0])[0]
        return int(hit[0]) if hit.size else self.m


def greedy_rows(x, num_inducing, kernel, lengthscales=None, linear=None, floor=0.0):
    """The greedy rows of ``x`` (n x d, device, float64) under ``kernel`` (an ``RBFKernel`` / ``DenseMaternKernel``; its noise
    is not used): m = min(n, ``num_inducing``) rows, nothing read back.  ``lengthscales`` and ``linear`` follow
    ``Sparse.SparseBlock``: per-dimension length-scales beside a kernel at l = 1 (the selection runs on x / l), and the
    variances v_e of a linear term in the units of ``x`` (on x / l its weights are v l^2).  A kernel that itself has
    per-dimension length-scales stands for its unit twin with ``lengthscales`` = its ``l``.  ``floor``: a pivot residual at
    or below it ends the rank count and leaves a zero column."""
    if not isinstance(kernel, (RBFKernel, DenseMaternKernel)):
        raise TypeError('greedy_rows takes an RBFKernel or a DenseMaternKernel, got %s' % type(kernel).__name__)
    if x.dim() != 2 or x.dtype != torch.float64:
        raise ValueError('greedy selection is built for float64 inputs (n x d) only')
    if int(num_inducing) < 1:
        raise ValueError('num_inducing must be at least 1')
    floor = non_negative(floor, 'floor', finite=True)
    if kernel.ard:
        if lengthscales is not None:
            raise ValueError('lengthscales beside a kernel that has its own per-dimension length-scales')
        kernel, lengthscales = kernel.with_values(1.0, kernel.sf, kernel.noise), kernel.l
    cov = BlockCovariance(kernel, x, lengthscales, linear)
    n = int(x.shape[0])
    m = min(n, int(num_inducing))
    rows, factor, diag, trace, rank = devi.pivoted_cholesky(cov.inputs(x).contiguous(), m, kernel.l, kernel.sf, cov.lin, floor,
                                                            cov=kernel.cov)
    return GreedyRows(n, rows, factor, diag, trace, rank)


def select_inducing(X, num_inducing, lengthscale=1., variance=1., nu=None, linear_variance=None, ARD=False, tol=None, preprocess=True,
                    dtype='f64', device=None):
    """``(Z, rows, trace)`` for the host array ``X`` (n x d): the greedy rows under the covariance a plugin constructed with
    the same (``lengthscale``, ``variance``, ``nu``, ``linear_variance``, ``ARD``) starts from, ``Z = X[rows]`` in the
    caller's units, and trace[j] = tr(K - Q_j) for j = 0 .. len(rows).  ``preprocess``: the selection runs on the z-scored
    inputs, exactly as ``RegressionMethod._preprocess`` forms them, which is where the plugins' length-scales live.
    ``tol``: keep only the first m' rows, the smallest m' <= ``num_inducing`` with trace[m'] <= tol * trace[0].
    ``SGP_FITC(Z=select_inducing(X, 1000, ...)[0])``, and the same for every other inducing-point plugin."""
    if int(num_inducing) < 1:
        raise ValueError('num_inducing must be at least 1')
    if dev.as_torch_dtype(dtype) != torch.float64:
        raise ValueError("greedy selection is built for dtype 'f64' only (FP32 cannot hold the residual's cancellation)")
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('X must be an n x d matrix')
    if not np.isfinite(X).all():
        raise ValueError('X must be finite')
    d = X.shape[1]
    ell = lengthscale_argument(lengthscale, bool(ARD), strict=True)
    sf = positive_scalar(variance, 'variance')
    linear = None
    if linear_variance is not None:
        linear = per_dimension(linear_variance, d, 'linear_variance')
        if not (np.isfinite(linear).all() and (linear > 0).all()):
            raise ValueError('linear_variance must be positive and finite, got %r' % (linear_variance,))
    if tol is not None:
        tol = non_negative(tol, 'tol', finite=True)
    lengthscales = per_dimension(ell, d, 'lengthscale') if ARD else None
    kernel = (RBFKernel(l=1.0 if ARD else ell, sf=sf) if nu is None
              else DenseMaternKernel(nu=nu, l=1.0 if ARD else ell, sf=sf))
    inputs = (X - X.mean(axis=0)) / X.std(axis=0) if preprocess else X
    device = dev.require_gpu(device)
    picked = greedy_rows(dev.to_device(inputs, torch.float64, device), num_inducing, kernel, lengthscales, linear)
    rows, trace = picked.rows_numpy(), picked.trace_numpy()
    if tol is not None:
        hit = np.nonzero(trace <= tol * trace[0])[0]
        keep = max(1, int(hit[0])) if hit.size else picked.m
        rows, trace = rows[:keep], trace[:keep + 1]
    return X[rows], rows, trace
