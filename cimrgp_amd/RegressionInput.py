"""The regression plugins: the drop-in boundary of the package.

``RegressionMethod`` mirrors the reference's plugin base class
(RegressionInput.py:10-52): ``fit(train_data=[X, Y]) -> bool`` and
``predict(test_data) -> ndarray`` with column-wise z-scoring of inputs and
labels (population std) done by the base class.  Nine plugins stand on it, over two bases:

    PosteriorQueries          a plugin that holds one fitted block: predict_with_variance and the five further queries
                              (predictive_gradients, leave_one_out, loo_log_predictive_density, predict_with_covariance,
                              posterior_samples_f), each written once; a plugin whose block does not answer the five names
                              the reason in ``unsupported`` and they raise TypeError, from one place
      GP_RBF, GP_Matern       the exact GP (Posteriors.DenseBlock)
      InducingPointMethod     a plugin with m inducing inputs Z: their draw or z-scoring, the upload of X, Y, Z, ``inducing_inputs``
                              after the fit, the ARD rule of the covariance, and the queries' ``budget_bytes`` of the chunked blocks
        SparseGP              FITC / VFE (Sparse.SparseBlock); SGP_FITC and SparseGP_RBF fix the approximation,
                              SparseGP_RBFLinear adds the reference's linear term
        SVIGP_RBF             variational, Student-t likelihood (SVGP.SVGPBlock)
        BGPLVM                uncertain (Gaussian) inputs (Psi.UncertainInputBlock)

The constructors and ``_fit`` check their arguments through four functions (``positive_scalar``, ``non_negative``,
``lengthscale_argument``, ``per_dimension``).

``GP_RBF`` replaces the
GPy-backed subclass (RegressionInput.py:55-67) with the HIP kernels: isotropic
RBF (GPy defaults l = 1, variance = 1 on the z-scored inputs), Gaussian noise
``labels.var() * 0.01`` on the z-scored labels.  ``optimize=True`` reproduces the
``model.optimize()`` step (RegressionInput.py:63): L-BFGS-B (SciPy, the optimiser GPy's
default ``'lbfgsb'`` wraps) on the log marginal likelihood over (variance, length-scale,
noise), all constrained positive through a log transform, starting from those defaults;
objective and gradient are evaluated on the GPU (one Cholesky, K^-1 = L^-T L^-1 through the
MFMA kernels, one fused reduction for the gradient).  Default is fixed hyper-parameters.

``GP_Matern`` is the same plugin with a half-integer Matern covariance (nu = 1/2, 3/2, 5/2;
GPy's ``Matern32(variance, lengthscale)`` is ``GP_Matern(1.5, lengthscale, variance)``): it
differs from ``GP_RBF`` only in the kernel object ``_make_kernel`` builds, whose ``cov`` selects
the covariance of every Gram, gradient and prediction kernel.
"""
import abc

import numpy as np
import torch

from . import device as dev
from ._lib import COV_RBF
from .Hyper import (append_linear, maximize_elbo, minimize_lml, pack_posterior, pack_theta, posterior_gradient, scaled, split_linear,
                    unit_lengthscale, unpack_posterior, unpack_theta)
from .KernelClass import RBFKernel, DenseMaternKernel
from .Posteriors import DenseBlock, NOISE_FRACTION, joint_run


def log_marginal_likelihood(x, y, ell, sf, noise, cov=COV_RBF, want_grad=True):
    """One block's LML of targets y (device, n x q) under K = k_cov(x, x) (length-scale ell, variance sf) + noise I, and
    its gradient w.r.t. (log sf, log ell, log noise) as a NumPy (3,) array: Gram, factorisation, solve, log-determinant,
    K^-1 = L^-T L^-1 (row-wise solve of the identity, SYRK) and the fused gradient reduction.  ``ell`` a (d,) vector (ARD):
    the same on x / ell at unit length-scale, and the gradient is w.r.t. (log sf, log l_1 .. log l_d, log noise), (d + 2,).
    Raises LinAlgError if K is not PD.  ``GP_RBF.log_marginal_likelihood`` and the MRGP layer objective for blocks the
    batched call (cimrgp_layer_lml_grad_cov) cannot take both run this."""
    ard = np.ndim(ell) > 0
    if ard:
        x, ell = unit_lengthscale(x, ell)[1], 1.0
    n, q = y.shape
    kbuf = dev.rbf_gram(x, ell, sf, noise, lower_only=True, cov=cov)
    ws, info = dev.potrf(kbuf, n)
    alpha = y.clone()
    dev.potrs(kbuf, n, ws, alpha)
    dev.raise_if_not_pd(info)
    half_logdet = float(dev.logdet_half(kbuf, n).item())
    fit = float((y * alpha).sum().item())
    lml = -0.5 * fit - q * half_logdet - 0.5 * n * q * np.log(2 * np.pi)
    if not want_grad:
        return lml, None
    # K^-1 = U U^T with U = L^-T: the identity carried through the row-wise solve, then a SYRK
    u = dev.alloc_matrix(n, n, x.dtype, x.device)
    u.zero_()
    u[:n, :n].fill_diagonal_(1.0)
    dev.trsm_rows(kbuf, n, ws, u, n)
    kinv = dev.alloc_matrix(n, n, x.dtype, x.device)
    kinv.zero_()
    dev.syrk_lower(kinv, u, n, n)            # lower(kinv) = -K^-1
    kinv.neg_()
    if ard:
        grad = dev.lml_grad_ard(x, kinv, n, alpha, sf, noise, cov=cov)
    else:
        grad = dev.lml_grad(x, kinv, n, alpha, ell, sf, noise, cov=cov)
    return lml, grad.cpu().numpy()


# ---- the argument checks of the constructors and of ``_fit`` ---------------------------------------------------------------
def positive_scalar(value, what):
    """``value`` as a float: one positive finite number."""
    if np.ndim(value) != 0 or not (np.isfinite(value) and value > 0):
        raise ValueError('%s must be a positive number, got %r' % (what, value))
    return float(value)


def non_negative(value, what, finite=False):
    """``value`` as a float: a number >= 0 (NaN is refused, and with ``finite`` infinity); ``what`` names it in the message."""
    if not value >= 0 or (finite and not np.isfinite(value)):
        raise ValueError('%s must not be negative' % what)
    return float(value)


def lengthscale_argument(lengthscale, ard, strict=False):
    """A constructor's ``lengthscale``: a float, or a 1-d float64 array (one entry per input dimension), which needs ``ard``.
    With ``ard`` the plugin builds its kernel at l = 1, which cannot refuse the values itself: they are checked here,
    positive and finite in every entry.  ``strict``: they are checked first and in any case (``BGPLVM``, which takes no
    other covariance), else a scalar without ``ard`` is left to the kernel."""
    ls = np.asarray(lengthscale, dtype=np.float64)
    bad = ls.size == 0 or not (np.isfinite(ls).all() and (ls > 0).all())
    if strict and (ls.ndim > 1 or bad):
        raise ValueError('lengthscale must be positive and finite in every entry, got %r' % (lengthscale,))
    if ls.ndim > 0 and not ard:
        raise ValueError('a sequence of length-scales needs ARD=True')
    if ls.ndim > 1:
        raise ValueError('lengthscale must be a scalar or a sequence with one entry per input dimension')
    if ard and bad:
        raise ValueError('lengthscale must be positive and finite in every entry, got %r' % (lengthscale,))
    return ls.copy() if ls.ndim else float(ls)


def per_dimension(value, d, what=None):
    """``value`` as a fresh (d,) float64 vector: a scalar stands for every dimension.  ``what`` names a vector that must
    have d entries (else its length is left to the block's own check)."""
    if np.ndim(value) == 0:
        return np.full(d, float(value))
    value = np.array(value, dtype=np.float64)
    if what is not None and value.shape[0] != d:
        raise ValueError('%s has %d entries, the inputs have %d dimensions' % (what, value.shape[0], d))
    return value


class RegressionMethod(object):
    __metaclass__ = abc.ABCMeta

    def __init__(self):
        self.preprocess = True

    def _preprocess(self, data, train):
        """Zero-mean, unit-variance normalisation by default."""
        if train:
            inputs, labels = data
            self.data_mean = inputs.mean(axis=0)
            self.data_std = inputs.std(axis=0)
            self.labels_mean = labels.mean(axis=0)
            self.labels_std = labels.std(axis=0)
            return ((inputs - self.data_mean) / self.data_std,
                    (labels - self.labels_mean) / self.labels_std)
        return (data - self.data_mean) / self.data_std

    def _reverse_trans_labels(self, labels):
        return labels * self.labels_std + self.labels_mean

    def fit(self, train_data):
        if self.preprocess:
            train_data = self._preprocess(train_data, True)
        return self._fit(train_data)

    def predict(self, test_data):
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        labels = self._predict(test_data)
        if self.preprocess:
            labels = self._reverse_trans_labels(labels)
        return labels

    @abc.abstractmethod
    def _fit(self, train_data):
        """Fit the model. Return True if successful"""
        return True

    @abc.abstractmethod
    def _predict(self, test_data):
        """Predict on test data"""
        return None


class PosteriorQueries(RegressionMethod):
    """The posterior queries of a plugin that holds one fitted block (``GP_RBF``: a DenseBlock, ``SparseGP``: a
    SparseBlock), written once: the z-scoring in and out, the chain rule through ``data_std`` / ``labels_std``, the
    symmetric covariance from its lower triangle, the (size, q, ns) reshape of the samples and the Gaussian log density.
    A plugin keeps ``block`` (None before ``fit``), ``_y`` (the fit's z-scored labels on the device), ``dtype``, and
    supplies ``_joint``; ``_accumulates`` says whether the block's ``predict`` / ``predict_grad`` add into their outputs
    (which are then zeroed first) or overwrite them; ``_test_inputs`` and ``_grad_scale`` are overridden by the plugin
    that rescales its inputs itself.  The public methods here have the exact plugin's signatures; keyword arguments that
    a plugin's own public methods add (``budget_bytes``, ``include_noise``) go to the block's method unchanged.
    ``unsupported``: why the plugin's block does not answer the five queries beyond ``predict`` /
    ``predict_with_variance`` (they raise TypeError, fitted or not), or None."""
    _accumulates = False
    unsupported = None

    def _fitted_block(self, what):
        if self.block is None:
            raise RuntimeError('call fit() before %s()' % what)
        return self.block

    def _refuse_unsupported(self, what):
        """The first step of each of the five further queries; ``what``: the public method that was called."""
        if self.unsupported is not None:
            raise TypeError('%s() of %s (%s) is not yet supported' % (what, self.name, self.unsupported))

    def _variance_shape(self, ns):
        """The shape of the predictive variance at ``ns`` test inputs: one per input, shared by the outputs."""
        return (ns,)

    def _test_inputs(self, test_data):
        """The (preprocessed) test inputs on the block's device, in the block's units."""
        return dev.to_device(np.atleast_2d(np.asarray(test_data, dtype=np.float64)), self.dtype, self.block.x.device)

    def _grad_scale(self):
        """d (block's inputs) / d (preprocessed inputs) per dimension where the plugin rescales them, else None."""
        return None

    def _joint(self, blk, xs, cov_out=None, samples=None, seed=0):
        """Add the joint predictive covariance at ``xs`` to ``cov_out``'s lower triangle, or draws to ``samples``."""
        raise NotImplementedError

    def _outputs(self, shape, device):
        return (torch.zeros if self._accumulates else torch.empty)(shape, dtype=self.dtype, device=device)

    def _predict(self, test_data):
        return self._predict_mean_var(test_data, want_var=False)[0]

    def _predict_mean_var(self, test_data, want_var, **block_kw):
        blk = self._fitted_block('predict')
        xs = self._test_inputs(test_data)
        mean = self._outputs((xs.shape[0], self._y.shape[1]), xs.device)
        var = self._outputs(self._variance_shape(xs.shape[0]), xs.device) if want_var else None
        blk.predict(xs, mean, var, **block_kw)
        return mean.double().cpu().numpy(), None if var is None else var.double().cpu().numpy()

    def _predict_with_variance(self, test_data, **block_kw):
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        mean, var = self._predict_mean_var(test_data, True, **block_kw)
        if self.preprocess:
            mean = self._reverse_trans_labels(mean)
        return mean, var

    def predict_with_variance(self, test_data):
        """Mean (un-z-scored) and latent predictive variance (in z-scored label units
        times labels_std^2 per column is left to the caller; returned as is)."""
        return self._predict_with_variance(test_data)

    def _predictive_gradients(self, test_data, **block_kw):
        self._refuse_unsupported('predictive_gradients')
        blk = self._fitted_block('predictive_gradients')
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        xs = self._test_inputs(test_data)
        ns, d = int(xs.shape[0]), int(xs.shape[1])
        mean_grad = self._outputs((ns, d, int(self._y.shape[1])), xs.device)
        var_grad = self._outputs((ns, d), xs.device)
        blk.predict_grad(xs, mean_grad, var_grad, **block_kw)
        dmu, dvar = mean_grad.double().cpu().numpy(), var_grad.double().cpu().numpy()
        s = self._grad_scale()
        if s is not None:
            dmu = dmu * s[None, :, None]
            dvar = dvar * s[None, :]
        if self.preprocess:
            inv_std = 1.0 / np.asarray(self.data_std, dtype=np.float64)
            dmu = dmu * inv_std[None, :, None] * np.asarray(self.labels_std, dtype=np.float64)[None, None, :]
            dvar = dvar * inv_std[None, :]
        return dmu, dvar

    def predictive_gradients(self, test_data):
        """GPy's ``predictive_gradients``: ``(dmu_dX (N*, d, q), dvar_dX (N*, d))`` with respect to the original test
        inputs (the chain rule through the input z-scoring and, with ARD, the per-dimension 1 / lengthscale scaling).  The
        mean gradient is in the original label units, per output; the variance gradient is left in z-scored label units,
        as ``predict_with_variance`` leaves the variance."""
        return self._predictive_gradients(test_data)

    def _loo_z(self, what, **block_kw):
        """(labels, LOO mean, LOO variance) in the (z-scored) units of the fit, NumPy, for the public method ``what``."""
        self._refuse_unsupported(what)
        blk = self._fitted_block('leave_one_out')
        y = self._y
        mean = torch.empty_like(y)
        var = torch.empty(y.shape[0], dtype=self.dtype, device=y.device)
        blk.loo(y, mean, var, **block_kw)
        return y.double().cpu().numpy(), mean.double().cpu().numpy(), var.double().cpu().numpy()

    def _leave_one_out(self, **block_kw):
        _, mean, var = self._loo_z('leave_one_out', **block_kw)
        if self.preprocess:
            mean = self._reverse_trans_labels(mean)
        return mean, var

    def leave_one_out(self):
        """Closed-form leave-one-out prediction of every training label from the other n - 1 (Rasmussen & Williams
        5.4.2; hyper-parameters and noise as fitted): ``(mean (n, q), var (n,))``.  The mean is in the original label
        units; the variance is left in z-scored label units, as ``predict_with_variance`` leaves it, but includes the
        noise: it is the variance of an observation."""
        return self._leave_one_out()

    def _loo_log_predictive_density(self, **block_kw):
        y, mean, var = self._loo_z('loo_log_predictive_density', **block_kw)
        q = y.shape[1]
        return -0.5 * q * np.log(2 * np.pi * var) - 0.5 * ((y - mean) ** 2).sum(axis=1) / var

    def loo_log_predictive_density(self):
        """(n,) log densities of each training label under its leave-one-out predictive Gaussian, in z-scored label
        units, summed over the outputs; their sum is the LOO-CV score (R&W eq. 5.11)."""
        return self._loo_log_predictive_density()

    def predict_with_covariance(self, test_data):
        """Mean (un-z-scored) and the latent joint predictive covariance (N* x N*, z-scored label units like
        ``predict_with_variance``'s variance, which is its diagonal)."""
        self._refuse_unsupported('predict_with_covariance')
        blk = self._fitted_block('predict_with_covariance')
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        mean, _ = self._predict_mean_var(test_data, want_var=False)
        xs = self._test_inputs(test_data)
        ns = int(xs.shape[0])
        cov = torch.zeros((ns, ns), dtype=self.dtype, device=xs.device)
        self._joint(blk, xs, cov_out=cov)
        cov = torch.tril(cov) + torch.tril(cov, -1).t()
        if self.preprocess:
            mean = self._reverse_trans_labels(mean)
        return mean, cov.double().cpu().numpy()

    def posterior_samples_f(self, test_data, size=1, seed=0):
        """``size`` draws (size, N*, q) of the latent function in the original label units: the z-scored draw
        mean + chol(Sigma + 1e-6 sf2 I) Z (Z_c = phi(seed, 0, c, .), c = sample * q + output; include/cimrgp_joint.h)
        times labels_std, plus labels_mean, per output."""
        self._refuse_unsupported('posterior_samples_f')
        blk = self._fitted_block('posterior_samples_f')
        if int(size) < 1:
            raise ValueError('size must be at least 1')
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        mean, _ = self._predict_mean_var(test_data, want_var=False)
        ns, q = mean.shape
        xs = self._test_inputs(test_data)
        out = torch.zeros((int(size) * q, ns), dtype=self.dtype, device=xs.device)
        self._joint(blk, xs, samples=out, seed=int(seed))
        f = mean[None, :, :] + out.double().cpu().numpy().reshape(int(size), q, ns).transpose(0, 2, 1)
        if self.preprocess:
            f = f * self.labels_std + self.labels_mean
        return f


class GP_RBF(PosteriorQueries):
    name = 'GP_RBF'

    def __init__(self, lengthscale=1., variance=1., dtype='f64', device=None, optimize=True, max_iters=1000, ARD=False):
        """``ARD=True``: one length-scale per input dimension (GPy's ``RBF(ARD=True)``, which the
        reference's comparison script fits, scripts/tests/GPRBF_vs_ciMRGP_vs_fiMRGP.py:118; the plugin
        itself is ``ARD=False``, RegressionInput.py:60).  Inputs are divided by their length-scales
        and every kernel then runs with unit length-scale; ``self.lengthscales`` holds the vector.
        ``optimize=True`` (default) is the reference's behaviour: its ``_fit`` always calls
        ``model.optimize()`` (RegressionInput.py:63).  ``optimize=False`` keeps the starting
        hyper-parameters (GPy's defaults l = 1, variance = 1, noise = 1 % of the label variance):
        the opt-in fast path, and the definition of the fixed-parameter parity target."""
        super(GP_RBF, self).__init__()
        self._initial = (float(lengthscale), float(variance))
        self.ARD = bool(ARD)
        self.lengthscales = None             # ARD: (d,) vector after fit
        self.kernel = self._make_kernel(lengthscale, variance)
        self.dtype = dev.as_torch_dtype(dtype)
        self.device = device
        self.block = None
        self.optimize = optimize
        self.max_iters = max_iters
        self.optimizer_result = None

    def _make_kernel(self, l, sf, noise=None):
        """The plugin's covariance object (the one hook of a subclass with another covariance)."""
        return RBFKernel(l=l, sf=sf, noise=noise)

    # ---- log marginal likelihood and its gradient, on the GPU ----------------------------
    def log_marginal_likelihood(self, x, y, ell, sf, noise, want_grad=True):
        """LML of targets y (device, n x q) under K = sf E(ell) + noise I, and its gradient
        w.r.t. (log sf, log ell, log noise); ``ell`` a (d,) vector: ARD.  Raises LinAlgError if K is not PD."""
        return log_marginal_likelihood(x, y, ell, sf, noise, self.kernel.cov, want_grad)

    def log_marginal_likelihood_ard(self, x, y, ells, sf, noise):
        """ARD twin of :meth:`log_marginal_likelihood`: ``ells`` (d,) length-scales; gradient w.r.t.
        (log sf, log l_1 .. log l_d, log noise)."""
        return self.log_marginal_likelihood(x, y, np.asarray(ells, dtype=np.float64), sf, noise)

    def _optimize(self, x, y, noise0):
        """L-BFGS-B over [log sf, log l (ARD: one per dimension), log noise] from the kernel's values; sets
        ``optimizer_result``, ``kernel`` (ARD: at l = 1.0) and, under ARD, ``lengthscales``."""
        n_ell = int(x.shape[1]) if self.ARD else None
        theta0 = pack_theta(self.kernel.sf, [self.kernel.l] * n_ell if self.ARD else self.kernel.l, noise0)

        def objective(theta):
            return self.log_marginal_likelihood(x, y, *unpack_theta(theta, n_ell))

        res = minimize_lml(objective, theta0, self.max_iters)
        self.optimizer_result = res
        ell, sf, noise = unpack_theta(res.x, n_ell)
        if self.ARD:
            self.lengthscales, ell = ell, 1.0
        self.kernel = self._make_kernel(ell, sf, noise)

    def _fit(self, train_data):
        inputs, labels = train_data
        device = dev.require_gpu(self.device)
        inputs = np.atleast_2d(np.asarray(inputs, dtype=np.float64))
        labels = np.atleast_2d(np.asarray(labels, dtype=np.float64))
        # every fit starts from the constructor's values (a re-fit does not start from the
        # previous optimum); the noise of the plugin is a property of the (z-scored) labels as a whole
        self.kernel = self._make_kernel(self._initial[0], self._initial[1])
        self.kernel.noise = float(labels.var()) * NOISE_FRACTION
        x = dev.to_device(inputs, self.dtype, device)
        y = dev.to_device(labels, self.dtype, device)
        if self.optimize:
            self._optimize(x, y, self.kernel.noise)
        elif self.ARD:
            self.lengthscales = per_dimension(self.kernel.l, x.shape[1])
            self.kernel = self._make_kernel(1.0, self.kernel.sf, self.kernel.noise)
        if self.ARD:
            self._scale, x = unit_lengthscale(x, self.lengthscales)          # unit length-scale from here on
        self.block = DenseBlock(x, self.kernel)
        zero_bias = torch.zeros(y.shape[1], dtype=self.dtype, device=device)
        sink = torch.zeros_like(y)
        self.block.fit(y, None, sink, shared_bias=zero_bias)
        dev.raise_if_not_pd(self.block.info)
        self._y = y                                      # the (z-scored) labels: leave_one_out reads them
        return True

    # ---- what PosteriorQueries asks of the plugin ----------------------------------------------
    _accumulates = True                  # DenseBlock.predict / predict_grad add into their outputs

    def _test_inputs(self, test_data):
        """ARD: divided by the length-scales here, the block runs at unit length-scale."""
        xs = super(GP_RBF, self)._test_inputs(test_data)
        return scaled(xs, self._scale) if self.ARD else xs

    def _grad_scale(self):
        return 1.0 / np.asarray(self.lengthscales, dtype=np.float64) if self.ARD else None

    def _joint(self, blk, xs, cov_out=None, samples=None, seed=0):
        joint_run(blk.joint_call(0, 0, xs.shape[0]), blk.kernel, xs, 0, False, cov_out, samples, seed)

class GP_Matern(GP_RBF):
    """``GP_RBF`` with the Matern covariance of smoothness ``nu`` in {0.5, 1.5, 2.5}
    (:class:`~cimrgp_amd.KernelClass.DenseMaternKernel`): the same z-scoring, noise rule,
    L-BFGS-B optimisation of the log-transformed (variance, length-scale(s), noise), ARD and
    ``predict_with_variance``.  GPy's ``Matern32(input_dim, variance, lengthscale)`` maps to
    ``GP_Matern(1.5, lengthscale, variance)``, ``Matern52`` to ``nu = 2.5``."""
    name = 'GP_Matern'

    def __init__(self, nu=1.5, lengthscale=1., variance=1., dtype='f64', device=None, optimize=True, max_iters=1000, ARD=False):
        DenseMaternKernel(nu)                # ValueError for an unsupported nu, before anything else
        self.nu = float(nu)
        super(GP_Matern, self).__init__(lengthscale, variance, dtype, device, optimize, max_iters, ARD)

    def _make_kernel(self, l, sf, noise=None):
        return DenseMaternKernel(nu=self.nu, l=l, sf=sf, noise=noise)


class InducingPointMethod(PosteriorQueries):
    """A plugin whose block stands on m = ``num_inducing`` inducing inputs.  ``Z=None`` draws them from the z-scored
    training inputs (:meth:`inducing_draw`; ``inducing_ids`` then holds the rows); a given ``Z`` (m x d) is in the caller's
    units and is z-scored with the inputs.  After the fit ``inducing_inputs`` holds Z in the caller's units.  A subclass
    sets ``ARD`` and, for a Matern covariance, ``nu``; its ``_fit`` goes through :meth:`_upload` and
    :meth:`_publish_inducing_inputs`, its ``_block`` through :meth:`_covariance`.  Every such block predicts in chunks, so
    the public queries here take ``budget_bytes``, the work area of a chunk."""
    nu = None

    def __init__(self, num_inducing, Z, seed, jitter, device):
        super(InducingPointMethod, self).__init__()
        if int(num_inducing) < 1:
            raise ValueError('num_inducing must be at least 1')
        self.num_inducing = int(num_inducing)
        self.Z = None if Z is None else np.atleast_2d(np.asarray(Z, dtype=np.float64))
        self.seed, self.jitter, self.device = seed, float(jitter), device
        self.block = self.optimizer_result = None
        self.lengthscales = None             # ARD: (d,) vector after fit
        self.inducing_ids = None             # rows of the training set drawn as inducing inputs (Z=None)
        self.inducing_inputs = None          # Z of the fitted model, in the caller's units

    def _make_kernel(self, l, sf, noise=None):
        if self.nu is None:
            return RBFKernel(l=l, sf=sf, noise=noise)
        return DenseMaternKernel(nu=self.nu, l=l, sf=sf, noise=noise)

    def _covariance(self, ell, sf, noise=None):
        """``(kernel, the block's keyword arguments)`` at (ell, sf, noise).  ARD: ``ell`` is the (d,) vector, which the block
        takes as ``lengthscales=`` beside a kernel at l = 1; else the kernel is at ``ell``."""
        if self.ARD:
            return self._make_kernel(1.0, sf, noise), dict(lengthscales=ell)
        return self._make_kernel(ell, sf, noise), {}

    def inducing_draw(self, n):
        """The documented draw of inducing rows among n training rows."""
        return np.random.RandomState(self.seed).permutation(n)[:min(n, self.num_inducing)]

    def _inducing_inputs(self, inputs):
        """Z in the (z-scored) units of ``inputs``."""
        if self.Z is None:
            self.inducing_ids = self.inducing_draw(inputs.shape[0])
            return inputs[self.inducing_ids]
        self.inducing_ids = None
        if self.Z.shape[1] != inputs.shape[1]:
            raise ValueError('Z must have the dimension of the inputs')
        return (self.Z - self.data_mean) / self.data_std if self.preprocess else self.Z

    def _upload(self, train_data):
        """The first step of a fit: forget the block, leave the (z-scored) inputs, labels and inducing inputs on the device
        as ``_x``, ``_y``, ``_z``.  Returns ``(inputs, labels, d)``, the host arrays as float64 matrices."""
        inputs, labels = train_data
        device = dev.require_gpu(self.device)
        inputs = np.atleast_2d(np.asarray(inputs, dtype=np.float64))
        labels = np.atleast_2d(np.asarray(labels, dtype=np.float64))
        self.block = None
        self._x = dev.to_device(inputs, self.dtype, device)
        self._y = dev.to_device(labels, self.dtype, device)
        self._z = dev.to_device(self._inducing_inputs(inputs), self.dtype, device)
        return inputs, labels, inputs.shape[1]

    def _publish_inducing_inputs(self):
        """The last step of a fit: ``inducing_inputs``, Z (as fitted: it may have been learned) in the caller's units."""
        z = self._z.double().cpu().numpy()
        self.inducing_inputs = z * self.data_std + self.data_mean if self.preprocess else z

    # ---- the posterior queries: PosteriorQueries', with the block's own keyword arguments -----------------------
    def predict_with_variance(self, test_data, include_noise=False, budget_bytes=None):
        """Mean (un-z-scored) and predictive variance, left in z-scored label units as ``GP_RBF.predict_with_variance``
        leaves it (latent; ``include_noise`` adds the noise).  ``budget_bytes``: work area of the chunked prediction."""
        return self._predict_with_variance(test_data, include_noise=include_noise, budget_bytes=budget_bytes)

    def predictive_gradients(self, test_data, budget_bytes=None):
        """``GP_RBF.predictive_gradients`` for the sparse posterior: ``(dmu_dX (N*, d, q), dvar_dX (N*, d))`` with respect
        to the original test inputs.  The mean gradient is in the original label units, the variance gradient in z-scored
        label units, as ``predict_with_variance`` leaves the variance (:meth:`~cimrgp_amd.Sparse.SparseBlock.predict_grad`;
        ARD's 1 / lengthscale is applied by the block)."""
        return self._predictive_gradients(test_data, budget_bytes=budget_bytes)

    def leave_one_out(self, budget_bytes=None):
        """Closed-form leave-one-out prediction of every training label from the other n - 1 under the fitted sparse
        model (exact for FITC's covariance Q_ff + Lambda; VFE / DTC: the same formula with Lambda = noise I):
        ``(mean (n, q), var (n,))``, at the cost of one prediction pass over the training set.  The mean is in the original
        label units; the variance is left in z-scored label units and includes the noise, as ``GP_RBF.leave_one_out``'s."""
        return self._leave_one_out(budget_bytes=budget_bytes)

    def loo_log_predictive_density(self, budget_bytes=None):
        """(n,) log densities of each training label under its leave-one-out predictive Gaussian, in z-scored label
        units, summed over the outputs; their sum scores the fit -- and the choice of m -- without a held-out set."""
        return self._loo_log_predictive_density(budget_bytes=budget_bytes)


class SparseGP(InducingPointMethod):
    """Inducing-point GP regression plugin (:class:`~cimrgp_amd.Sparse.SparseBlock`): ``approximation='fitc'`` or
    ``'vfe'``, cost n m^2 for m = ``num_inducing`` inducing inputs.  ``Z=None`` draws them from the z-scored training
    inputs, ``numpy.random.RandomState(seed).permutation(n)[:min(n, num_inducing)]``; a given ``Z`` (m x d) is in the
    caller's units and is z-scored with the inputs.  ``nu`` in {0.5, 1.5, 2.5} selects the Matern covariance, None the
    RBF.  The noise is ``labels.var() * 0.01`` on the z-scored labels, as for ``GP_RBF``.  ``optimize=True``: L-BFGS-B
    over (log variance, log length-scale, log noise) with Z fixed, on SciPy's own two-point differences of the
    GPU-evaluated objective; the default keeps the starting values, as the reference's sparse plugins do.
    ``jac='analytic'`` gives L-BFGS-B the analytic gradient instead (:meth:`~cimrgp_amd.Sparse.SparseBlock.lml_grad`: one
    call per step instead of four evaluations); ``optimize_inducing=True`` (needs ``optimize=True, jac='analytic'``) also
    learns Z, as GPy's ``SparseGPRegression`` does: the parameter vector is [log sf, log l, log noise, Z.ravel()] with Z in
    the z-scored units of the fit.  After the fit ``inducing_inputs`` holds Z in the caller's units.  With a Matern 1/2
    covariance the objective has a kink wherever an inducing input sits on a training input or on another inducing input
    (Z drawn from the data starts there); the gradient takes dk/dz = 0 at r = 0 and the combination is not refused.
    ``ARD=True``: one length-scale per input dimension, as the reference's sparse plugins have it (gpflow's and GPy's
    ``RBF(d, ARD=True)``; DESIGN.md, "ARD length-scales for the sparse GP").  ``lengthscale`` is then a scalar (every
    dimension) or a length-d sequence; after the fit ``lengthscales`` holds the (d,) vector in z-scored input units and
    ``kernel.l`` is 1.0, as for ``GP_RBF(ARD=True)``.  ``ell=`` of :meth:`log_marginal_likelihood` and
    :meth:`log_marginal_likelihood_grad` takes a scalar or a (d,) vector, and the optimisers' parameter vector is
    [log sf, log l_1 .. log l_d, log noise, (Z.ravel())]."""
    name = 'SparseGP'

    def __init__(self, num_inducing=1000, approximation='fitc', lengthscale=1., variance=1., nu=None, Z=None, seed=0, jitter=1e-6,
                 dtype='f64', device=None, optimize=False, max_iters=200, jac='2-point', optimize_inducing=False, ARD=False):
        from .Sparse import APPROXIMATIONS
        if str(approximation).lower() not in APPROXIMATIONS:
            raise ValueError("approximation must be 'fitc' or 'vfe', got %r" % (approximation,))
        super(SparseGP, self).__init__(num_inducing, Z, seed, jitter, device)
        if jac not in ('2-point', 'analytic'):
            raise ValueError("jac must be '2-point' or 'analytic', got %r" % (jac,))
        if optimize_inducing and not (optimize and jac == 'analytic'):
            raise ValueError("optimize_inducing=True needs optimize=True and jac='analytic'")
        self.jac = jac
        self.optimize_inducing = bool(optimize_inducing)
        self.approximation = str(approximation).lower()
        self.nu = None if nu is None else float(nu)
        self.ARD = bool(ARD)
        self._initial = (lengthscale_argument(lengthscale, self.ARD), float(variance))
        self.kernel = self._covariance(*self._initial)[0]          # ValueError for an unsupported nu
        self.dtype = dev.as_torch_dtype(dtype)
        self.optimize = optimize
        self.max_iters = max_iters
        self.linear_variances = None         # SparseGP_RBFLinear: (d,) variances of the linear term after fit
        self._initial_linear = None          # ... and their starting value, a scalar or a (d,) vector

    def _block(self, ell, sf, noise, linear=None):
        """The block at (ell, sf, noise) (:meth:`_covariance`).  A model with a linear term carries its variances:
        ``linear``, or the fitted ones."""
        from .Sparse import SparseBlock
        kernel, kw = self._covariance(ell, sf, noise)
        if linear is None:
            linear = self.linear_variances
        if linear is not None:
            kw['linear'] = linear
        return SparseBlock(self._x, self._z, kernel, self.approximation, self.jitter, **kw)

    def _set_covariance(self, ell, sf, noise):
        """``kernel`` and, under ARD, ``lengthscales`` of the model at (ell, sf, noise)."""
        self.kernel, kw = self._covariance(ell, sf, noise)
        self.lengthscales = kw.get('lengthscales')

    def _ell(self, ell=None):
        """The ``ell=`` argument of the two objective calls: the fitted value by default; ARD: a scalar stands for all
        dimensions."""
        if not self.ARD:
            return self.kernel.l if ell is None else float(ell)
        return self.lengthscales if ell is None else per_dimension(ell, self.lengthscales.shape[0])

    def _block_at(self, ell, sf, noise, linear):
        """The block of the two objective calls: at their arguments, each the fitted value by default.  ``linear``: the (d,)
        variances of the linear term, a scalar standing for all dimensions; refused by a model without the term."""
        if linear is not None:
            if self.linear_variances is None:
                raise TypeError('%s has no linear term' % type(self).__name__)
            linear = per_dimension(linear, self.linear_variances.shape[0])
        k = self.kernel
        return self._block(self._ell(ell), k.sf if sf is None else float(sf), k.noise if noise is None else float(noise), linear)

    def log_marginal_likelihood(self, ell=None, sf=None, noise=None, linear=None):
        """The FITC marginal likelihood / the VFE bound of the fitted data at (ell, sf, noise); the fitted values by
        default.  Raises LinAlgError if a factorisation fails or a lambda_i is not positive.  ``linear``: the variances of
        the linear term of a model that has one (``SparseGP_RBFLinear``)."""
        blk = self._fitted_block('log_marginal_likelihood')
        if ell is None and sf is None and noise is None and linear is None:
            return blk.log_marginal_likelihood()
        return self._block_at(ell, sf, noise, linear).fit(self._y).log_marginal_likelihood()

    def log_marginal_likelihood_grad(self, ell=None, sf=None, noise=None, want_z=True, linear=None):
        """``(lml, dtheta, dZ)`` of the fitted data at (ell, sf, noise), the fitted values by default: the objective of
        :meth:`log_marginal_likelihood`, its gradient w.r.t. (log sf, log ell, log noise) as a (3,) array (ARD: one entry
        per length-scale, (d + 2,)) and, with ``want_z``, w.r.t. the inducing inputs in the (z-scored) units of the fit as
        an (m, d) array, else None.  A model with a linear term has d more entries at the end of dtheta, w.r.t.
        (log v_1 .. log v_d), taken at ``linear`` (default: the fitted variances).
        Raises as :meth:`log_marginal_likelihood` does."""
        self._fitted_block('log_marginal_likelihood_grad')
        lml, dtheta, dz = self._block_at(ell, sf, noise, linear).lml_grad(self._y, want_z=want_z)
        return lml, dtheta, None if dz is None else dz.double().cpu().numpy()

    def _optimize(self, noise0):
        """L-BFGS-B over [log sf, log l (ARD: one per dimension), log noise] and, with ``optimize_inducing``, Z: on the
        analytic gradient (``jac='analytic'``) or on SciPy's two-point differences of the objective.  Returns the
        optimum's (ell, sf, noise).  A model with a linear term learns its d log-variances too, between log noise and Z, and
        leaves the optimum's in ``linear_variances``."""
        analytic, learn_z = self.jac == 'analytic', self.optimize_inducing
        n_ell = self.lengthscales.shape[0] if self.ARD else None
        theta0 = pack_theta(self.kernel.sf, self.lengthscales if self.ARD else self.kernel.l, noise0)
        n_lin = 0 if self.linear_variances is None else self.linear_variances.shape[0]
        if n_lin:
            theta0 = append_linear(theta0, self.linear_variances)
        nt = theta0.shape[0]
        zshape = tuple(self._z.shape)
        if learn_z:
            theta0 = np.concatenate([theta0, self._z.double().cpu().numpy().ravel()])

        def objective(theta):
            if learn_z:
                self._z = dev.to_device(theta[nt:].reshape(zshape), self.dtype, self._x.device)
            blk = self._block(*unpack_theta(theta, n_ell), linear=split_linear(theta, n_lin, n_ell)[1] if n_lin else None)
            if not analytic:
                return blk.fit(self._y).log_marginal_likelihood()
            lml, dtheta, dz = blk.lml_grad(self._y, want_z=learn_z)
            return lml, dtheta if dz is None else np.concatenate([dtheta, dz.double().cpu().numpy().ravel()])

        res = minimize_lml(objective, theta0, self.max_iters, jac=True if analytic else None)
        if learn_z:
            self._z = dev.to_device(res.x[nt:].reshape(zshape), self.dtype, self._x.device)
        self.optimizer_result = res
        if n_lin:
            self.linear_variances = split_linear(res.x, n_lin, n_ell)[1]
        return unpack_theta(res.x, n_ell)

    def _fit(self, train_data):
        ell, sf = self._initial
        d = np.atleast_2d(np.asarray(train_data[0])).shape[1]          # a wrong length is refused before the device is asked for
        if self.ARD:
            ell = per_dimension(ell, d, 'lengthscale')
        if self._initial_linear is not None:
            self.linear_variances = per_dimension(self._initial_linear, d, 'linear_variance')
        _, labels, _ = self._upload(train_data)
        self._set_covariance(ell, sf, float(labels.var()) * NOISE_FRACTION)
        if self.optimize:
            self._set_covariance(*self._optimize(self.kernel.noise))
        self.block = self._block(self._ell(), self.kernel.sf, self.kernel.noise).fit(self._y)
        self._publish_inducing_inputs()
        return True

    def _joint(self, blk, xs, cov_out=None, samples=None, seed=0):
        blk.joint(xs, cov_out=cov_out, samples=samples, seed=seed)


class SGP_FITC(SparseGP):
    """The reference's ``SGP_FITC`` plugin: :class:`SparseGP` with ``approximation='fitc'``."""
    name = 'SGP_FITC'

    def __init__(self, num_inducing=1000, lengthscale=1., variance=1., nu=None, Z=None, seed=0, jitter=1e-6, dtype='f64',
                 device=None, optimize=False, max_iters=200, jac='2-point', optimize_inducing=False, ARD=False):
        super(SGP_FITC, self).__init__(num_inducing, 'fitc', lengthscale, variance, nu, Z, seed, jitter, dtype, device, optimize,
                                       max_iters, jac, optimize_inducing, ARD)


class SparseGP_RBF(SparseGP):
    """The reference's ``SparseGP_RBF`` plugin: :class:`SparseGP` with ``approximation='vfe'``, the bound GPy's
    ``SparseGPRegression`` optimises, with the RBF (or Matern) covariance alone; the reference's ``RBF + Linear`` kernel is
    :class:`SparseGP_RBFLinear`."""
    name = 'SparseGP_RBF'

    def __init__(self, num_inducing=1000, lengthscale=1., variance=1., nu=None, Z=None, seed=0, jitter=1e-6, dtype='f64',
                 device=None, optimize=False, max_iters=200, jac='2-point', optimize_inducing=False, ARD=False):
        super(SparseGP_RBF, self).__init__(num_inducing, 'vfe', lengthscale, variance, nu, Z, seed, jitter, dtype, device, optimize,
                                           max_iters, jac, optimize_inducing, ARD)


class SparseGP_RBFLinear(SparseGP):
    """The reference's ``SparseGP_RBF`` plugin with the kernel the reference gives it, ``RBF(d, ARD=True) + Linear(d, ARD=True)``
    under GPy's ``SparseGPRegression`` (the VFE bound): k(x, x') = k_cov(x, x') + sum_e v_e x_e x'_e on the z-scored inputs
    ("A linear term for the sparse GP").  The linear term lets the model extrapolate a trend in the labels, which a
    stationary covariance can only soak up in a long length-scale.  ``linear_variance``: the starting v, a scalar (every
    dimension) or a length-d sequence; after the fit ``linear_variances`` holds the (d,) vector.  ``optimize=True`` learns
    them with the other hyper-parameters: the parameter vector is [log sf, log l .., log noise, log v_1 .. log v_d,
    (Z.ravel())].  Everything else is :class:`SparseGP`'s, ``nu`` and ``approximation='fitc'`` included.  The five posterior
    queries beyond ``predict`` / ``predict_with_variance`` are not built for this kernel and raise TypeError."""
    name = 'SparseGP_RBFLinear'
    unsupported = 'a covariance with a linear term'

    def __init__(self, num_inducing=1000, lengthscale=1., variance=1., linear_variance=1., nu=None, Z=None, seed=0, jitter=1e-6,
                 dtype='f64', device=None, optimize=False, max_iters=200, jac='2-point', optimize_inducing=False, ARD=True,
                 approximation='vfe'):
        super(SparseGP_RBFLinear, self).__init__(num_inducing, approximation, lengthscale, variance, nu, Z, seed, jitter, dtype,
                                                 device, optimize, max_iters, jac, optimize_inducing, ARD)
        v = np.asarray(linear_variance, dtype=np.float64)
        if v.ndim > 1 or v.size == 0 or not (np.isfinite(v).all() and (v > 0).all()):
            raise ValueError('linear_variance must be positive and finite, a scalar or one entry per input dimension, got %r'
                             % (linear_variance,))
        self._initial_linear = float(v) if v.ndim == 0 else v.copy()


class SVIGP_RBF(InducingPointMethod):
    """The reference's ``SVIGP_RBF`` plugin: GPy's ``SVGP`` with the kernel ``RBF(ARD) + Linear(ARD) + White(0.01)`` and a
    Student-t likelihood (``deg_free`` = 3), optimised on the full batch, predicting the latent function
    (:class:`~cimrgp_amd.SVGP.SVGPBlock`; DESIGN.md, "Variational sparse GP with a Student-t likelihood").  It is the one
    plugin whose fit a few gross outliers do not drag.  Inputs and labels are z-scored; ``Z`` follows :class:`SparseGP`'s
    rule and stays fixed; the likelihood's scale starts at 0.01 (the labels are z-scored); ``white_variance`` is fixed.
    ``optimize=True`` (the reference's behaviour): L-BFGS-B with the analytic gradient over [log sf, log l .., log s2,
    log v .., mu.ravel(), vech(P) per output], started from the optimal Gaussian posterior of the VFE fit at the initial
    hyper-parameters; ``optimize=False`` keeps those hyper-parameters and that posterior.  ``likelihood='gaussian'``,
    ``ARD=False``, ``linear=False`` and ``nu`` (a Matern covariance) leave the reference's model.  After the fit:
    ``lengthscales`` ((d,) under ARD, else None), ``linear_variances``, ``likelihood_scale``, ``optimizer_result`` and
    ``params``, the optimiser's whole vector.  Float32 and the five posterior queries beyond ``predict`` /
    ``predict_with_variance`` are not built and raise TypeError."""
    name = 'SVIGP_RBF'
    INITIAL_SCALE = 0.01
    unsupported = 'a variational posterior'

    def __init__(self, num_inducing=100, lengthscale=1., variance=1., linear_variance=1., white_variance=0.01,
                 likelihood='student_t', deg_free=3., nu=None, Z=None, seed=0, jitter=1e-6, dtype='f64', device=None, optimize=True,
                 max_iters=1000, ARD=True, linear=True):
        from .SVGP import LIKELIHOODS
        if str(likelihood).lower() not in LIKELIHOODS:
            raise ValueError("likelihood must be 'student_t' or 'gaussian', got %r" % (likelihood,))
        super(SVIGP_RBF, self).__init__(num_inducing, Z, seed, jitter, device)
        self._initial = (positive_scalar(lengthscale, 'lengthscale'), positive_scalar(variance, 'variance'),
                         positive_scalar(linear_variance, 'linear_variance'))
        self.deg_free = positive_scalar(deg_free, 'deg_free')
        self.white_variance = non_negative(white_variance, 'white_variance and jitter', finite=True)
        non_negative(jitter, 'white_variance and jitter')
        self.dtype = dev.as_torch_dtype(dtype)
        if self.dtype != torch.float64:
            raise TypeError("%s with dtype='f32' is not yet supported" % self.name)
        self.nu = None if nu is None else float(nu)
        self.kernel = self._make_kernel(1.0, variance)           # ValueError for an unsupported nu
        self.likelihood, self.optimize, self.max_iters = str(likelihood).lower(), optimize, max_iters
        self.ARD, self.linear = bool(ARD), bool(linear)
        self.linear_variances = self.likelihood_scale = self.params = None

    def _block(self, theta):
        """The block at theta = [log sf, log l (1, or d under ARD), log s2, (log v_1 .. log v_d)]."""
        from .SVGP import SVGPBlock
        d = int(self._x.shape[1])
        n_ell = d if self.ARD else None
        head, lin, _ = split_linear(np.asarray(theta, dtype=np.float64), d if self.linear else 0, n_ell)
        ell, sf, s2 = unpack_theta(head, n_ell)
        kernel, kw = self._covariance(ell, sf)
        return SVGPBlock(self._x, self._z, kernel, self.likelihood, self.deg_free, s2, self.white_variance, self.jitter,
                         linear=lin if self.linear else None, **kw)

    def _vfe_posterior(self, theta):
        """(mu (q, m), P (q, m, m)) of the optimal Gaussian q(v) at ``theta``: P = L_B and mu = L_B^-T gamma of the VFE fit
        with noise s2, on the same L_u (the white variance rides in the fit's jitter)."""
        from .Sparse import SparseBlock
        blk = self._block(theta)
        k, m, q = blk.kernel, blk.m, int(self._y.shape[1])
        vfe = SparseBlock(self._x, self._z, self._make_kernel(k.l, k.sf, blk.scale), 'vfe', self.jitter + self.white_variance / k.sf,
                          lengthscales=blk.lengthscales, linear=blk.linear).fit(self._y)
        lb = torch.tril(vfe.lb[:m, :m])
        mu = torch.linalg.solve_triangular(lb.t(), vfe.gamma, upper=True)
        return mu.t().double().cpu().numpy(), np.repeat(lb.double().cpu().numpy()[None], q, axis=0)

    def _elbo_grad(self, theta, mu, p):
        """``SVGPBlock.elbo_grad`` in NumPy."""
        to = lambda a: dev.to_device(a, self.dtype, self._x.device)
        f, dtheta, dmu, dp = self._block(theta).elbo_grad(self._y, to(mu), to(p))
        return f, dtheta, dmu.double().cpu().numpy(), dp.double().cpu().numpy()

    def _split(self, params):
        nt = self._n_theta
        q, m = int(self._y.shape[1]), int(self._z.shape[0])
        params = np.asarray(params, dtype=np.float64)
        if params.shape != self.params.shape:
            raise ValueError('params must have the %d entries of the fitted vector' % self.params.shape[0])
        return (params[:nt],) + unpack_posterior(params[nt:], q, m)

    def elbo_grad(self, params=None):
        """``(F, gradient)`` of the evidence lower bound of the fitted data at ``params`` (default: the fitted ``params``):
        the whole vector [log sf, log l .., log s2, (log v ..), mu.ravel(), vech(P) per output, log-diagonal] and the
        analytic gradient w.r.t. it.  Raises LinAlgError as :meth:`~cimrgp_amd.SVGP.SVGPBlock.elbo_grad` does."""
        self._fitted_block('elbo_grad')
        theta, mu, p = self._split(self.params if params is None else params)
        f, dtheta, dmu, dp = self._elbo_grad(theta, mu, p)
        return f, np.concatenate([dtheta, posterior_gradient(dmu, dp, p)])

    def elbo(self, params=None):
        """The evidence lower bound of :meth:`elbo_grad`."""
        self._fitted_block('elbo')
        return self.elbo_grad(params)[0]

    def _fit(self, train_data):
        d = self._upload(train_data)[2]
        device = self._x.device
        ell0, sf0, lin0 = self._initial
        theta = pack_theta(sf0, per_dimension(ell0, d) if self.ARD else ell0, self.INITIAL_SCALE)
        if self.linear:
            theta = append_linear(theta, per_dimension(lin0, d))
        self._n_theta = theta.shape[0]
        mu, p = self._vfe_posterior(theta)
        if self.optimize:
            self.optimizer_result, theta, mu, p = maximize_elbo(self._elbo_grad, theta, mu, p, self.max_iters)
        self.params = np.concatenate([theta, pack_posterior(mu, p)])
        blk = self._block(theta)
        self.kernel, self.lengthscales, self.linear_variances = blk.kernel, blk.lengthscales, blk.linear
        self.likelihood_scale = blk.scale
        self.block = blk.set_posterior(dev.to_device(mu, self.dtype, device), dev.to_device(p, self.dtype, device))
        self._publish_inducing_inputs()
        return True

    def _variance_shape(self, ns):
        """The latent variance differs between the outputs: each has its own q(v_c)."""
        return (ns, int(self._y.shape[1]))

    def predict_with_variance(self, test_data, budget_bytes=None):
        """Mean (un-z-scored, the latent mean, as the reference predicts: ``include_likelihood=False``) and the latent
        variance per output (ns, q), left in z-scored label units as the other plugins leave it.  ``budget_bytes``: work
        area of the chunked prediction."""
        return self._predict_with_variance(test_data, budget_bytes=budget_bytes)


class BGPLVM(InducingPointMethod):
    """The reference's ``BGPLVM`` plugin: gpflow's ``BayesianGPLVM`` used as a sparse VFE regression whose inputs are not
    points but Gaussians x_i ~ N(inputs_i, diag X_var_i) (:class:`~cimrgp_amd.Psi.UncertainInputBlock`; DESIGN.md, "Sparse GP
    regression on uncertain inputs").  The defaults are the reference's: ``num_inducing`` = 100 rows drawn as
    :meth:`InducingPointMethod.inducing_draw` draws them, the unit RBF with one length-scale per dimension (``ARD=True``), gpflow's
    likelihood variance ``noise`` = 1.0 (on the z-scored labels), ``X_var=None`` = ``inputs.var() * 0.01`` over all entries of
    the z-scored inputs, and no optimisation.  ``X_var``: the variances of the inputs in the caller's (squared) units, a
    scalar, a (d,) vector or an (n, d) array, checked finite and not negative; it is scaled with the z-scoring.  A scalar or
    a vector takes the shared-variance route (existing covariance and matrix-core calls), an (n, d) array the psi kernels
    (cimrgp_psi1, cimrgp_psi2).  ``optimize=True``: L-BFGS-B over [log sf, log l_1 .. log l_d, log noise] (one log l without
    ARD) on SciPy's two-point differences of the bound, Z and the inputs' distributions fixed.  After the fit:
    ``lengthscales`` ((d,) under ARD, else None), ``inducing_inputs`` (Z in the caller's units), ``kernel``,
    ``optimizer_result``.  ``predict(test, test_var=)`` takes uncertain test inputs too.  Float32, the five posterior
    queries beyond ``predict`` / ``predict_with_variance`` and the variance at uncertain test inputs are not built and
    raise TypeError."""
    name = 'BGPLVM'
    X_VAR_FRACTION = 0.01
    unsupported = 'uncertain inputs'

    def __init__(self, num_inducing=100, X_var=None, noise=1.0, lengthscale=1., variance=1., ARD=True, Z=None, seed=0, jitter=1e-6,
                 device=None, optimize=False, max_iters=200):
        super(BGPLVM, self).__init__(num_inducing, Z, seed, jitter, device)
        noise, variance = positive_scalar(noise, 'noise'), positive_scalar(variance, 'variance')
        self.ARD = bool(ARD)
        self._initial = (lengthscale_argument(lengthscale, self.ARD, strict=True), variance, noise)
        non_negative(jitter, 'jitter')
        if X_var is not None:
            X_var = np.asarray(X_var, dtype=np.float64)
            if X_var.ndim > 2 or not (np.isfinite(X_var).all() and (X_var >= 0).all()):
                raise ValueError('X_var must be a scalar, a (d,) vector or an (n, d) array of finite variances, none negative')
        self.X_var, self.optimize, self.max_iters = X_var, optimize, max_iters
        self.dtype = torch.float64
        self.kernel = self._covariance(*self._initial)[0]

    def _variances(self, var, rows, d, what):
        """``var`` (the caller's units; a scalar, (d,) or (rows, d)) in the z-scored units: a host (d,) vector, or a
        (rows, d) device tensor."""
        var = np.asarray(var, dtype=np.float64)
        if var.ndim > 2 or (var.ndim == 1 and var.shape != (d,)) or (var.ndim == 2 and var.shape != (rows, d)):
            raise ValueError('%s must be a scalar, a (%d,) vector or a (%d, %d) array, got shape %r' % (what, d, rows, d, var.shape))
        if not (np.isfinite(var).all() and (var >= 0).all()):
            raise ValueError('%s must be finite and not negative' % what)
        if self.preprocess:
            var = var / np.asarray(self.data_std, dtype=np.float64) ** 2
        if var.ndim == 2:
            return dev.to_device(var, self.dtype, self._x.device)
        return per_dimension(var, d)

    def _block(self, ell, sf, noise):
        """The block at (ell, sf, noise) (:meth:`_covariance`)."""
        from .Psi import UncertainInputBlock
        kernel, kw = self._covariance(ell, sf, noise)
        return UncertainInputBlock(self._x, self._var, self._z, kernel, self.jitter, **kw)

    def _fit(self, train_data):
        ell, sf, noise = self._initial
        d = np.atleast_2d(np.asarray(train_data[0])).shape[1]          # a wrong length is refused before the device is asked for
        if self.ARD:
            ell = per_dimension(ell, d, 'lengthscale')
        inputs = self._upload(train_data)[0]
        if self.X_var is None:
            self._var = np.full(d, float(inputs.var()) * self.X_VAR_FRACTION)         # of the inputs as the model sees them
        else:
            self._var = self._variances(self.X_var, inputs.shape[0], d, 'X_var')
        if self.optimize:
            n_ell = d if self.ARD else None
            objective = lambda theta: self._block(*unpack_theta(theta, n_ell)).fit(self._y).bound()
            self.optimizer_result = minimize_lml(objective, pack_theta(sf, ell, noise), self.max_iters, jac=None)
            ell, sf, noise = unpack_theta(self.optimizer_result.x, n_ell)
        self.block = self._block(ell, sf, noise).fit(self._y)
        self.kernel, self.lengthscales = self.block.kernel, ell if self.ARD else None
        self._publish_inducing_inputs()
        return True

    def elbo(self):
        """The evidence lower bound of the fitted data, F - KL (z-scored units)."""
        return self._fitted_block('elbo').elbo()

    def kl_divergence(self):
        """KL(q(X) || N(0, I)) of the (z-scored) inputs' distributions: gpflow's default prior."""
        return self._fitted_block('kl_divergence').kl()

    def predict(self, test_data, test_var=None, budget_bytes=None):
        """The predictive mean; ``test_var`` (a scalar, (d,) or (ns, d), the caller's units): the test inputs are Gaussians
        N(test_data, diag test_var) and the mean is taken under them (Psi1 of the test inputs in place of K(X*, Z))."""
        blk = self._fitted_block('predict')
        if test_var is None:
            return super(BGPLVM, self).predict(test_data)
        test_data = np.atleast_2d(np.asarray(test_data, dtype=np.float64))
        xs_var = self._variances(test_var, test_data.shape[0], test_data.shape[1], 'test_var')
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        xs = self._test_inputs(test_data)
        mean = torch.empty((xs.shape[0], self._y.shape[1]), dtype=self.dtype, device=xs.device)
        blk.predict(xs, mean, None, budget_bytes=budget_bytes, xs_var=xs_var)
        mean = mean.double().cpu().numpy()
        return self._reverse_trans_labels(mean) if self.preprocess else mean

    def predict_with_variance(self, test_data, include_noise=False, test_var=None, budget_bytes=None):
        """Mean (un-z-scored) and predictive variance, left in z-scored label units as the other plugins leave it (latent;
        ``include_noise`` adds the noise).  With ``test_var`` the variance is not built: TypeError (:meth:`predict` gives
        the mean)."""
        if test_var is not None:
            raise TypeError('the predictive variance of %s at uncertain test inputs is not yet supported' % self.name)
        self._fitted_block('predict_with_variance')
        return self._predict_with_variance(test_data, include_noise=include_noise, budget_bytes=budget_bytes)
