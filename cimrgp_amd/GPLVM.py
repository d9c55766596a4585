"""``BayesianGPLVM``: the ``BGPLVM`` plugin optimised on the analytic gradient of its bound, with learned inducing inputs and
learned input distributions ("Gradients of the bound on uncertain inputs").  The gradient is
:meth:`~cimrgp_amd.Psi.UncertainInputBlock.elbo_grad`: the n m and n m^2 / 2 work is cimrgp_psi1_grad and cimrgp_psi2_grad
(include/cimrgp_psi_grad.h); the optimiser is ``Hyper.minimize_lml``.

The class is imported from this module and is NOT in ``cimrgp_amd.__all__``: the exported plugin classes and every public
method of each are pinned by the recorded-call tests, and ``BGPLVM`` itself keeps its signature and its device calls."""
import numpy as np
import torch

from . import device as dev
from .Hyper import minimize_lml, pack_theta, unpack_theta
from .RegressionInput import BGPLVM, per_dimension

INPUT_PRIORS = ('observed', 'standard')


class BayesianGPLVM(BGPLVM):
    """``BGPLVM`` with four more arguments.  ``jac``: 'analytic' (the default) optimises on ``elbo_grad``; '2-point' is the
    parent's path, SciPy's differences of the bound over the hyper-parameters alone.  ``optimize_inducing``: Z is learned.
    ``optimize_inputs``: the inputs' distributions q(x_i) = N(mu_i, diag s_i) are learned -- mu and log s of every entry whose
    variance ``X_var`` is positive; an entry with variance 0 is an observed input and stays fixed; a shared ``X_var`` (a
    scalar or a (d,) vector) becomes per-row.  Both need ``optimize=True`` and ``jac='analytic'``.  ``input_prior``:
    'observed' is the prior N(observed inputs, X_var) of each input, so that KL = 0 before the fit; 'standard' is N(0, 1) on
    the z-scored inputs, gpflow's default and the parent's ``kl_divergence``.

    ``optimize=True`` runs one L-BFGS-B over [log sf, log l (d under ARD), log noise, (Z.ravel()), (mu and then log s of the
    learned entries)], maximising F - KL.  After the fit: ``input_means`` and ``input_variances`` ((n, d), the caller's units),
    and ``inducing_inputs``, ``lengthscales``, ``kernel`` and ``optimizer_result`` as on the parent.  What the parent does not
    build -- float32, the five further posterior queries -- is not built here; the variance at uncertain test inputs, which
    the parent's ``predict_with_variance(test_var=)`` refuses (here too), is :meth:`predict_uncertain`."""
    name = 'BayesianGPLVM'

    def __init__(self, num_inducing=100, X_var=None, noise=1.0, lengthscale=1., variance=1., ARD=True, Z=None, seed=0, jitter=1e-6,
                 device=None, optimize=False, max_iters=200, jac='analytic', optimize_inducing=False, optimize_inputs=False,
                 input_prior='observed'):
        super(BayesianGPLVM, self).__init__(num_inducing, X_var, noise, lengthscale, variance, ARD, Z, seed, jitter, device, optimize,
                                            max_iters)
        if jac not in ('2-point', 'analytic'):
            raise ValueError("jac must be '2-point' or 'analytic', got %r" % (jac,))
        if input_prior not in INPUT_PRIORS:
            raise ValueError("input_prior must be 'observed' or 'standard', got %r" % (input_prior,))
        if (optimize_inducing or optimize_inputs) and not (optimize and jac == 'analytic'):
            raise ValueError("optimize_inducing and optimize_inputs need optimize=True and jac='analytic'")
        self.jac, self.input_prior = jac, input_prior
        self.optimize_inducing, self.optimize_inputs = bool(optimize_inducing), bool(optimize_inputs)
        self.input_means = self.input_variances = None
        self._prior = (None, None)

    def _block(self, ell, sf, noise):
        """The parent's block at the current Z and input distributions, with the inputs' prior."""
        from .Psi import UncertainInputBlock
        kernel, kw = self._covariance(ell, sf, noise)
        return UncertainInputBlock(self._x, self._var, self._z, kernel, self.jitter, prior_mean=self._prior[0], prior_var=self._prior[1],
                                   **kw)

    def _rows(self, var):
        """The input variances as an (n, d) device tensor."""
        if isinstance(var, torch.Tensor):
            return var
        return torch.as_tensor(var, dtype=self.dtype).to(self._x.device).expand(int(self._x.shape[0]), -1).contiguous()

    def _maximize_elbo(self, theta0, n_ell):
        """L-BFGS-B on the analytic gradient over [theta, (Z), (mu, log s of the entries with s > 0)]; leaves the optimum's Z
        and input distributions in ``_z``, ``_x`` and ``_var`` and returns its (ell, sf, noise)."""
        learn_z, learn_x = self.optimize_inducing, self.optimize_inputs
        device, nt, zshape = self._x.device, theta0.shape[0], tuple(self._z.shape)
        nz = int(np.prod(zshape)) if learn_z else 0
        parts = [theta0]
        if learn_z:
            parts.append(self._z.double().cpu().numpy().ravel())
        if learn_x:
            self._var = self._rows(self._var)
            mu0, s0 = self._x.double().cpu().numpy(), self._var.double().cpu().numpy()
            mask = s0 > 0
            nx = int(mask.sum())
            parts += [mu0[mask], np.log(s0[mask])]

        def place(vec):
            if learn_z:
                self._z = dev.to_device(vec[nt:nt + nz].reshape(zshape), self.dtype, device)
            if learn_x:
                mu, s = mu0.copy(), s0.copy()
                mu[mask], s[mask] = vec[nt + nz:nt + nz + nx], np.exp(vec[nt + nz + nx:])
                self._x, self._var = dev.to_device(mu, self.dtype, device), dev.to_device(s, self.dtype, device)

        def objective(vec):
            place(vec)
            f, dtheta, dz, dmu, ds = self._block(*unpack_theta(vec, n_ell)).fit(self._y).elbo_grad(want_z=learn_z, want_inputs=learn_x)
            grad = [dtheta]
            if learn_z:
                grad.append(dz.double().cpu().numpy().ravel())
            if learn_x:                                              # d / dlog s = s d / ds
                grad += [dmu.double().cpu().numpy()[mask], ds.double().cpu().numpy()[mask] * np.exp(vec[nt + nz + nx:])]
            return f, np.concatenate(grad)

        self.optimizer_result = minimize_lml(objective, np.concatenate(parts), self.max_iters)
        place(self.optimizer_result.x)
        return unpack_theta(self.optimizer_result.x, n_ell)

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
        if self.input_prior == 'observed':                              # N(observed inputs, X_var); an entry with s = 0 adds nothing
            rows = self._rows(self._var).double()
            self._prior = (self._x.double().clone(), torch.where(rows > 0, rows, torch.ones_like(rows)))
        else:
            self._prior = (None, None)
        if self.optimize:
            n_ell = d if self.ARD else None
            theta0 = pack_theta(sf, ell, noise)
            if self.jac == 'analytic':
                ell, sf, noise = self._maximize_elbo(theta0, n_ell)
            else:
                objective = lambda theta: self._block(*unpack_theta(theta, n_ell)).fit(self._y).bound()
                self.optimizer_result = minimize_lml(objective, theta0, self.max_iters, jac=None)
                ell, sf, noise = unpack_theta(self.optimizer_result.x, n_ell)
        self.block = self._block(ell, sf, noise).fit(self._y)
        self.kernel, self.lengthscales = self.block.kernel, ell if self.ARD else None
        self._publish_inducing_inputs()
        mu, s = self._x.double().cpu().numpy(), self._rows(self._var).double().cpu().numpy()
        std = np.asarray(self.data_std, dtype=np.float64) if self.preprocess else 1.0
        self.input_means = mu * std + self.data_mean if self.preprocess else mu
        self.input_variances = s * std ** 2
        return True

    def predict_uncertain(self, test_data, test_var, include_noise=False, budget_bytes=None):
        """``(mean, var)`` at the uncertain test inputs N(test_data, diag test_var); ``test_var``: a scalar, (d,) or (ns, d), in
        the caller's (squared) units.  The mean (ns, q) is un-z-scored, as ``predict(test_data, test_var=)`` returns it; the
        variance is (ns, q) -- the spread of the posterior mean over the input's distribution differs from output to output --
        and is left in z-scored label units, as ``predict_with_variance`` leaves it (latent; ``include_noise`` adds the noise)
        (:meth:`~cimrgp_amd.Psi.UncertainInputBlock.predict_moments`).  ``budget_bytes``: work area of the chunked
        prediction."""
        blk = self._fitted_block('predict_uncertain')
        test_data = np.atleast_2d(np.asarray(test_data, dtype=np.float64))
        xs_var = self._variances(test_var, test_data.shape[0], test_data.shape[1], 'test_var')
        if self.preprocess:
            test_data = self._preprocess(test_data, False)
        xs = self._test_inputs(test_data)
        mean = torch.empty((xs.shape[0], self._y.shape[1]), dtype=self.dtype, device=xs.device)
        var = torch.empty_like(mean)
        blk.predict_moments(xs, xs_var, mean, var, include_noise=include_noise, budget_bytes=budget_bytes)
        mean = mean.double().cpu().numpy()
        return self._reverse_trans_labels(mean) if self.preprocess else mean, var.double().cpu().numpy()

    def kl_divergence(self):
        """KL(q(X) || the inputs' prior) of the (z-scored) inputs' distributions (``input_prior``)."""
        return self._fitted_block('kl_divergence').kl()

    def elbo_grad(self):
        """``(F - KL, dtheta, dZ, dmu, ds)`` of the fitted model: the evidence lower bound and its analytic gradient w.r.t.
        (log sf, log l (d under ARD), log noise), the inducing inputs (m, d), and the inputs' means and variances (n, d), as NumPy
        arrays in the z-scored units of the fit."""
        f, dtheta, dz, dmu, ds = self._fitted_block('elbo_grad').elbo_grad()
        return (f, dtheta) + tuple(t.double().cpu().numpy() for t in (dz, dmu, ds))
