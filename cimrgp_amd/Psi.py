"""Sparse GP regression on uncertain inputs ("Sparse GP regression on uncertain inputs"): the collapsed bound of
gpflow's ``BayesianGPLVM`` used as a regression, its inputs Gaussians x_i ~ N(mu_i, diag s_i) instead of points.

It is the VFE bound of :class:`~cimrgp_amd.Sparse.SparseBlock` with K_fu, K_uf K_fu and sum_i k_ii replaced by the psi
statistics of the RBF covariance (include/cimrgp_psi.h): with K_uu + eps sf I = L_u L_u^T and noise s2,

    T = L_u^-1 Psi2 L_u^-T        B = I + T / s2 = L_B L_B^T        c = L_u^-1 Psi1^T Y / s2        gamma = L_B^-1 c
    F = -1/2 n q log(2 pi s2) - q sum log (L_B)_ii - 1/2 |Y|^2 / s2 + 1/2 |gamma|^2 - 1/2 q (psi0 - tr T) / s2,  psi0 = n sf
    KL = 1/2 sum_{i,e: s_ie > 0} (s_ie + mu_ie^2 - 1 - log s_ie)         (the prior N(0, 1) of every input; s_ie = 0: observed)
    mean* = W* gamma,  var* = sf - sum A*^2 + sum W*^2 (+ s2)             A* = K(X*, Z) L_u^-T, W* = A* L_B^-T

so prediction is ``SparseBlock.predict`` on the factors built here.  Two routes give the psi statistics:

    per-row variances   ``x_var`` an (n, d) device tensor           cimrgp_psi1, cimrgp_psi2: the n m^2 / 2 exponentials
    a shared variance   ``x_var`` a scalar or a (d,) vector         Psi1 = cimrgp_cov_cross on inputs scaled by (l^2 + s)^-1/2;
                                                                    Psi2 = sf^2 prod_e (1 + 2 s_e / l_e^2)^-1/2 C o (G^T G) with
                                                                    G = cimrgp_cov_cross on inputs scaled by (l^2 + 2 s)^-1/2,
                                                                    G^T G = cimrgp_wsyrk_tn (w = 1) on the matrix cores and
                                                                    C_jk = exp(-sum_e (z_je - z_ke)^2 s_e / (2 l_e^2 (l_e^2 + 2 s_e)))

The n x m and n x m^2 work is those C calls; torch holds the buffers and does the m x m and m x q plumbing.

``bound_grad`` / ``elbo_grad`` give the analytic gradient of F (and F - KL) w.r.t. the hyper-parameters, Z and the inputs'
means and variances ("Gradients of the bound on uncertain inputs"): the weights dF/dPsi1, dF/dPsi2 and dF/dK_uu are
m x m torch algebra on the fit's factors, their contractions cimrgp_psi1_grad, cimrgp_psi2_grad (include/cimrgp_psi_grad.h)
and the covariance's pair contraction.  By either route of the fit the gradient takes the per-row kernels.

``predict_moments`` gives the predictive mean and variance at uncertain TEST inputs ("Predictive variance at
uncertain test inputs"): the law of total variance over the input's distribution, whose n m^2 / 2 exponentials are
cimrgp_psi2_rows_quad (include/cimrgp_psi_rows.h) -- a row's own Psi2 contracted with two weights and never stored.
"""
import numpy as np
import torch

from . import device as dev
from . import device_psi as devp
from ._lib import COV_RBF
from .Hyper import scaled
from .Sparse import SparseBlock, read_back


def _not_built(what):
    raise TypeError('%s of a block with uncertain inputs is not yet supported' % what)


def _between(lu, inner):
    """L_u^-T inner L_u^-1 for a symmetric ``inner`` (m x m), symmetrised; ``lu``: L_u as a lower-triangular tensor."""
    half = torch.linalg.solve_triangular(lu.t(), inner, upper=True)
    full = torch.linalg.solve_triangular(lu.t(), half.t().contiguous(), upper=True)
    return 0.5 * (full + full.t())


class UncertainInputBlock(SparseBlock):
    """Device-resident state of one sparse block whose training inputs are Gaussians: L_u, L_B, gamma as a
    :class:`~cimrgp_amd.Sparse.SparseBlock` keeps them ('vfe'), built from the psi statistics."""

    def __init__(self, x_mean, x_var, z, kernel, jitter=1e-6, lengthscales=None, prior_mean=None, prior_var=None):
        """``x_mean`` (n x d), ``z`` (m x d): float64 device tensors in the same units; ``kernel``: an ``RBFKernel`` with its
        ``noise`` set; ``lengthscales``: as for ``SparseBlock`` (ARD; ``kernel.l`` must then be 1.0).  ``x_var``: the
        variances of the inputs in the squared units of ``x_mean`` -- a scalar or a (d,) vector (every row has that
        variance: the shared-variance route, checked non-negative and finite here) or an (n, d) device tensor (the psi
        kernels; a negative or non-finite entry is found by the device and raises ValueError in :meth:`fit`).  A Matern
        covariance has no closed-form psi statistics and is refused, as are float32 blocks.  ``prior_mean``, ``prior_var``
        (gpflow's ``X_prior_mean`` and ``X_prior_var``): (n, d) device tensors, the prior N(prior_mean, diag prior_var) of the
        inputs that :meth:`kl` and :meth:`elbo_grad` are taken against; None: 0 and 1, gpflow's default."""
        if getattr(kernel, 'cov', None) != COV_RBF or not hasattr(kernel, 'with_noise'):
            raise TypeError('the psi statistics of %s are not yet supported (RBFKernel only)' % type(kernel).__name__)
        if x_mean.dtype != torch.float64:
            raise TypeError('a float32 block with uncertain inputs is not yet supported')
        SparseBlock.__init__(self, x_mean, z, kernel, 'vfe', jitter, lengthscales=lengthscales)
        self.x = self.x.contiguous()
        d = int(x_mean.shape[1])
        self.ell = np.full(d, float(kernel.l)) if self.lengthscales is None else self.lengthscales
        self._ell_dev = torch.as_tensor(self.ell, dtype=torch.float64).to(x_mean.device)
        self.x_var = self._variance(x_var, self.n, x_mean)
        self.prior_mean, self.prior_var = self._prior(prior_mean, 'prior_mean'), self._prior(prior_var, 'prior_var')
        self.bad = self._f_terms = self._fitted = None

    def _prior(self, t, what):
        """A prior's (n, d) tensor on the block's device, or None; the variances positive, both finite."""
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(self.x.shape):
            raise ValueError('%s must be an (n, d) tensor' % what)
        t = t.to(device=self.x.device, dtype=torch.float64).contiguous()
        if not bool(torch.isfinite(t).all()) or (what == 'prior_var' and not bool((t > 0).all())):
            raise ValueError('%s must be finite%s' % (what, ' and positive' if what == 'prior_var' else ''))
        return t

    @staticmethod
    def _variance(x_var, n, like):
        """``x_var`` as the block keeps it: a host float64 (d,) vector (shared), or an (n, d) device tensor."""
        d = int(like.shape[1])
        if isinstance(x_var, torch.Tensor) and x_var.dim() == 2:
            if tuple(x_var.shape) != (n, d) or x_var.dtype != like.dtype or x_var.device != like.device:
                raise ValueError('a per-row x_var must be an (n, d) tensor of the dtype and on the device of the inputs')
            return x_var.contiguous()
        v = x_var.detach().cpu().numpy() if isinstance(x_var, torch.Tensor) else x_var
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(d, float(v))
        if v.shape != (d,):
            raise ValueError('x_var must be a scalar, %d variances (one per input dimension) or an (n, %d) device tensor' % (d, d))
        if not (np.isfinite(v).all() and (v >= 0).all()):
            raise ValueError('x_var must be finite and not negative')
        return v

    # ---- the psi statistics -------------------------------------------------------------------------------------
    def _scaled_by(self, den):
        """(mu -> mu den^-1/2, Z den^-1/2) for a (d,) vector of denominators."""
        scale = torch.as_tensor(den ** -0.5, dtype=self.z.dtype, device=self.z.device)
        return (lambda t: scaled(t, scale)), scaled(self.z, scale)

    def _psi1(self, mu, var, out=None):
        """Psi1 of the rows ``mu`` with the variances ``var`` (a host (d,) vector or a device tensor of mu's shape)."""
        sf = self.kernel.sf
        if isinstance(var, torch.Tensor):
            return devp.psi1(mu.contiguous(), var.contiguous(), self.z, self._ell_dev, sf, out=out)
        l2 = self.ell ** 2
        to, zs = self._scaled_by(l2 + var)
        return dev.rbf_cross(to(mu), zs, 1.0, sf * float(np.prod(1.0 + var / l2) ** -0.5), out=out)

    def _psi2(self):
        """(lower(Psi2) in a padded m x m buffer, the device count of bad rows or None) of the training inputs."""
        n, m, sf, var = self.n, self.m, self.kernel.sf, self.x_var
        if isinstance(var, torch.Tensor):
            return devp.psi2(self.x, var, self.z, self._ell_dev, sf)
        l2 = self.ell ** 2
        den = l2 + 2.0 * var
        to, zs = self._scaled_by(den)
        g = dev.rbf_cross(to(self.x), zs, 1.0, 1.0)
        out = dev.wsyrk_tn(g, n, m, torch.ones(n, dtype=g.dtype, device=g.device))[0]
        zw = self.z * torch.as_tensor(np.sqrt(var / (2.0 * l2 * den)), dtype=self.z.dtype, device=self.z.device)
        c = torch.exp(-((zw[:, None, :] - zw[None, :, :]) ** 2).sum(dim=2))
        out[:m, :m] *= c * (sf * sf * float(np.prod(1.0 + 2.0 * var / l2) ** -0.5))
        return out, None

    # ---- the fit ------------------------------------------------------------------------------------------------
    def fit(self, y):
        """``y`` (n x q): targets on the device.  Nothing is read back but the two ``info`` words and the count of rows
        with a negative or non-finite variance: LinAlgError for a factor that is not positive definite, ValueError for
        such rows."""
        y = y.contiguous()
        k, n, m, q = self.kernel, self.n, self.m, int(y.shape[1])
        s2, dt, device = k.noise, self.z.dtype, self.z.device
        self.lu = self.cov.gram(self._zs, self.jitter * k.sf)
        self.ws_u, self.info_u = dev.potrf(self.lu, m)
        p1 = self._psi1(self.x, self.x_var)
        g = dev.wsyrk_tn(p1, n, m, torch.ones(n, dtype=dt, device=device), y)[1]          # Psi1^T Y (m x q)
        del p1
        p2, self.bad = self._psi2()
        # T = L_u^-1 Psi2 L_u^-T and c = L_u^-1 Psi1^T Y / s2: m x m and m x q, by substitution.  T is the step that limits
        # the accuracy of the whole fit (K_uu is ill-conditioned and the solve is two-sided); cimrgp_trsm_rows, built for
        # n >> m rows on the matrix cores, left T 3 .. 8 times further from its exact value here (DESIGN.md has the figures)
        low = torch.tril(p2[:m, :m])
        lu = torch.tril(self.lu[:m, :m])
        half = torch.linalg.solve_triangular(lu, low + torch.tril(low, -1).t(), upper=False)
        t = torch.linalg.solve_triangular(lu, half.t().contiguous(), upper=False)
        t = 0.5 * (t + t.t())
        self.lb = dev.alloc_matrix(m, m, dt, device)
        self.lb[:m, :m] = t / s2
        self.lb[:m, :m].diagonal().add_(1.0)
        self._enqueue_solve(torch.linalg.solve_triangular(lu, g / s2, upper=False).contiguous())
        self._fitted = (y, t)                              # what bound_grad() starts from beside the factors: Y and T
        self._f_terms = (dict(half_logdet_b=dev.logdet_half(self.lb, m), yy=(y.double() ** 2).sum(), gg=(self.gamma.double() ** 2).sum(),
                              tr_t=torch.diagonal(t).double().sum()), q)
        flags = dict(info_u=self.info_u, info_b=self.info_b)
        if self.bad is not None:
            flags['bad'] = self.bad
        h = read_back(flags, {})
        dev.raise_if_not_pd(h['info_u'])
        if h.get('bad', 0.0) > 0:
            raise ValueError('%d of the input rows have a negative or non-finite variance' % int(h['bad']))
        dev.raise_if_not_pd(h['info_b'])
        return self

    def bound(self):
        """F: the collapsed bound without the KL term.  At ``x_var`` = 0 it is the VFE bound of ``SparseBlock('vfe')``."""
        if self._f_terms is None:
            raise RuntimeError('call fit() before bound()')
        scalars, q = self._f_terms
        h = read_back(scalars, {})
        k, n = self.kernel, self.n
        return float(-0.5 * n * q * np.log(2 * np.pi * k.noise) - q * h['half_logdet_b'] - 0.5 * h['yy'] / k.noise + 0.5 * h['gg']
                     - 0.5 * q * (n * k.sf - h['tr_t']) / k.noise)

    log_marginal_likelihood = bound

    def kl(self):
        """KL(q(X) || N(0, I)) over the entries with a positive variance (s_ie = 0 is an observed input)."""
        var, mu = self.x_var, self.x.double()
        if self.prior_mean is not None or self.prior_var is not None:
            return float(self._kl_parts()[0].item())
        if isinstance(var, torch.Tensor):
            v = var.double()
            pos = v > 0
            safe = torch.where(pos, v, torch.ones_like(v))
            return float(0.5 * torch.where(pos, safe + mu ** 2 - 1.0 - torch.log(safe), torch.zeros_like(v)).sum().item())
        pos = var > 0
        if not pos.any():
            return 0.0
        cols = torch.as_tensor(np.nonzero(pos)[0]).to(mu.device)
        return float(0.5 * (self.n * (var[pos] - 1.0 - np.log(var[pos])).sum() + (mu.index_select(1, cols) ** 2).sum().item()))

    def elbo(self):
        return self.bound() - self.kl()

    def _rows_var(self):
        """``x_var`` as an (n, d) device tensor: a shared variance vector is broadcast."""
        var = self.x_var
        if isinstance(var, torch.Tensor):
            return var
        return torch.as_tensor(var, dtype=self.x.dtype).to(self.x.device).expand(self.n, -1).contiguous()

    def _kl_parts(self):
        """(KL, dKL/dmu, dKL/ds) against the prior on the device, float64: 1/2 [(s + (mu - m0)^2) / v0 - 1 - log(s / v0)] over
        the entries with s > 0; the gradients are zero at the others (observed inputs)."""
        v, mu = self._rows_var().double(), self.x.double()
        pm = torch.zeros_like(mu) if self.prior_mean is None else self.prior_mean
        pv = torch.ones_like(mu) if self.prior_var is None else self.prior_var
        pos = v > 0
        safe, zero = torch.where(pos, v, torch.ones_like(v)), torch.zeros_like(v)
        kl = 0.5 * torch.where(pos, (safe + (mu - pm) ** 2) / pv - 1.0 - torch.log(safe / pv), zero).sum()
        return kl, torch.where(pos, (mu - pm) / pv, zero), torch.where(pos, 0.5 * (1.0 / pv - 1.0 / safe), zero)

    # ---- the gradient of the bound ------------------------------------------------------------------------------
    def bound_grad(self, want_z=True, want_inputs=True):
        """After :meth:`fit`: ``(F, dtheta, dZ, dmu, ds)`` -- :meth:`bound`'s value, its gradient w.r.t. (log sf, log l, log
        noise) as a NumPy array (one log l, or d of them with ``lengthscales``), w.r.t. the inducing inputs (m x d) and
        w.r.t. the inputs' means and variances (n x d each), device tensors in the block's own input units, None where not
        wanted ("Gradients of the bound on uncertain inputs").  With P = Psi2, A = K_uu + P / s2 = L_u B L_u^T,
        u = L_B^-T gamma and v = L_u^-T u the weights are
            G1 = Y v^T / s2        G2 = L_u^-T [q / (2 s2) (I - B^-1) - u u^T / (2 s2)] L_u^-1
            G_uu = L_u^-T [q/2 (I - B^-1) - 1/2 u u^T - q / (2 s2) T] L_u^-1
        contracted by cimrgp_psi1_grad, cimrgp_psi2_grad and, for K_uu + eps sf I, the covariance's pair contraction.  The
        m x m solves are torch's, as in :meth:`fit`.  A shared variance vector is broadcast to (n, d) and takes the per-row
        kernels: ds is then per row, and the caller sums it over the rows."""
        if self._fitted is None:
            raise RuntimeError('call fit() before bound_grad()')
        y, t = self._fitted
        k, n, m, q = self.kernel, self.n, self.m, int(y.shape[1])
        s2, sf, dt, device = k.noise, k.sf, self.z.dtype, self.z.device
        f = self.bound()
        lu, lb = torch.tril(self.lu[:m, :m]), torch.tril(self.lb[:m, :m])
        eye = torch.eye(m, dtype=dt, device=device)
        u = torch.linalg.solve_triangular(lb.t(), self.gamma, upper=True)
        v = torch.linalg.solve_triangular(lu.t(), u, upper=True)
        lb_inv = torch.linalg.solve_triangular(lb, eye, upper=False)
        i_binv = eye - lb_inv.t() @ lb_inv
        uu = u @ u.t()

        between_lu = lambda inner: _between(lu, inner)
        g1 = (y @ v.t() / s2).contiguous()
        g2 = between_lu((0.5 * q / s2) * i_binv - uu / (2.0 * s2)).contiguous()
        guu = dev.alloc_matrix(m, m, dt, device)
        guu.zero_()
        guu[:m, :m] = between_lu(0.5 * q * i_binv - 0.5 * uu - (0.5 * q / s2) * t)
        var = self._rows_var()
        dmu, ds, dz, sums1 = devp.psi1_grad(self.x, var, self.z, self._ell_dev, sf, g1)
        del g1
        dmu2, ds2, dz2, sums2, bad = devp.psi2_grad(self.x, var, self.z, self._ell_dev, sf, g2)
        psums, _, dzu = self.cov.pair_grad(self._zs, self._zs, guu, want_z, scale=2.0)
        h = read_back(dict(tr_guu=torch.diagonal(guu[:m, :m]).double().sum(), tr_ib=torch.diagonal(i_binv).double().sum(),
                           uu=(u.double() ** 2).sum(), bad=bad, **self._f_terms[0]), dict(sums1=sums1, sums2=sums2, psums=psums))
        if h['bad'] > 0:
            raise ValueError('%d of the input rows have a negative or non-finite variance' % int(h['bad']))
        dsf = h['sums1'][0] + h['sums2'][0] + h['psums'][0] + self.jitter * sf * h['tr_guu'] - 0.5 * q * n * sf / s2
        dl = h['sums1'][1:] + h['sums2'][1:]
        dl = dl + h['psums'][1:] if self.lengthscales is not None else np.array([dl.sum() + h['psums'][1]])
        dnoise = (-0.5 * n * q + 0.5 * q * h['tr_ib'] + 0.5 * h['yy'] / s2 - 0.5 * h['gg'] - 0.5 * h['uu']
                  + 0.5 * q * (n * sf - h['tr_t']) / s2)
        dtheta = np.concatenate([[dsf], dl, [dnoise]])
        if want_z:
            dz = dz + dz2 + self.cov.chain_rule(dz=dzu)
        return f, dtheta, dz if want_z else None, dmu + dmu2 if want_inputs else None, ds + ds2 if want_inputs else None

    def elbo_grad(self, want_z=True, want_inputs=True):
        """:meth:`bound_grad` of F - KL: the KL term's gradient is taken from dmu and ds over the entries with s > 0."""
        f, dtheta, dz, dmu, ds = self.bound_grad(want_z, want_inputs)
        kl, kmu, ks = self._kl_parts()
        if want_inputs:
            dmu, ds = dmu - kmu.to(dmu.dtype), ds - ks.to(ds.dtype)
        return f - float(kl.item()), dtheta, dz, dmu, ds

    # ---- prediction ---------------------------------------------------------------------------------------------
    def predict(self, xs, mean=None, var=None, include_noise=False, budget_bytes=None, xs_var=None):
        """``SparseBlock.predict`` at exact test inputs.  ``xs_var`` (a scalar, a (d,) vector or an (ns, d) device
        tensor): the test inputs are Gaussians too and the mean is E_x* [k(x*, Z)] K_uu^-1 .. = Psi1* L_u^-T L_B^-T gamma;
        the variance at uncertain test inputs is (ns, q), not this method's (ns,): it is :meth:`predict_moments`', and
        ``var`` with ``xs_var`` stays refused here."""
        if xs_var is None:
            return SparseBlock.predict(self, xs, mean, var, include_noise, budget_bytes)
        if var is not None:
            _not_built('the predictive variance at uncertain test inputs')
        if self.gamma is None:
            raise RuntimeError('call fit() before predict()')
        sv = self._variance(xs_var, int(xs.shape[0]), xs)
        rows = (lambda s0, s1: sv[s0:s1]) if isinstance(sv, torch.Tensor) else (lambda s0, s1: sv)
        if mean is not None:
            cross = lambda s0, s1, out: self._psi1(xs[s0:s1], rows(s0, s1), out=out)
            for s0, s1, _, wstar in self._star_chunks(xs, budget_bytes, cross=cross):
                dev.sparse_tail(None, wstar, s1 - s0, self.m, self.gamma, self.kernel.sf, 0.0, mean[s0:s1], None, False)
        return mean, var

    def predict_moments(self, xs, xs_var, mean=None, var=None, include_noise=False, budget_bytes=None):
        """Predictive mean into ``mean`` and variance into ``var`` (both (ns, q) device tensors, either may be None) at the
        uncertain test inputs x*_i ~ N(xs_i, diag xs_var_i); ``xs_var``: a scalar, a (d,) vector or an (ns, d) device tensor
        ("Predictive variance at uncertain test inputs").  By the law of total variance, with
        C = L_u^-T (I - B^-1) L_u^-1, a = L_u^-T L_B^-T gamma and Psi2*_i the row's own Psi2,
            var_ic = sf - sum C o Psi2*_i  +  a_c^T Psi2*_i a_c - mean_ic^2   (+ noise with ``include_noise``)
        the latent variance averaged over the input, and the variance of the posterior mean over it, which depends on the
        output column.  C and a are m x m torch algebra on the fit's factors, once per call; the two contractions are
        cimrgp_psi2_rows_quad (include/cimrgp_psi_rows.h), chunk by chunk beside the mean, which is :meth:`predict`'s own
        path (the same bits as ``predict(xs, mean, xs_var=xs_var)`` for a per-row ``xs_var``).  A shared variance is
        broadcast to (ns, d) and takes the per-row kernels, as in :meth:`bound_grad`: a factorised shared route is not
        built.  A row's results do not depend on the chunking.  One host read at the end, the count of rows with a negative
        or non-finite variance: ValueError if there are any."""
        ns = int(xs.shape[0])
        sv = self._variance(xs_var, ns, xs)
        if self.gamma is None:
            raise RuntimeError('call fit() before predict_moments()')
        if not isinstance(sv, torch.Tensor):
            sv = torch.as_tensor(sv, dtype=xs.dtype).to(xs.device).expand(ns, -1).contiguous()
        if var is None:
            return self.predict(xs, mean, None, budget_bytes=budget_bytes, xs_var=sv)
        k, m, q, dt, device = self.kernel, self.m, int(self.gamma.shape[1]), self.z.dtype, self.z.device
        if mean is None:
            mean = torch.empty((ns, q), dtype=dt, device=device)
        lu, lb = torch.tril(self.lu[:m, :m]), torch.tril(self.lb[:m, :m])
        eye = torch.eye(m, dtype=dt, device=device)
        lb_inv = torch.linalg.solve_triangular(lb, eye, upper=False)
        c = _between(lu, eye - lb_inv.t() @ lb_inv).contiguous()
        a = torch.empty((m, q), dtype=dt, device=device)         # row-major whatever q is (a solve's (m, 1) result need not be)
        a.copy_(torch.linalg.solve_triangular(lu.t(), torch.linalg.solve_triangular(lb.t(), self.gamma, upper=True), upper=True))
        tr = torch.empty(ns, dtype=dt, device=device)
        bad, bad_chunk, scratch = torch.zeros(1, dtype=torch.float64, device=device), torch.empty(1, dtype=torch.float64, device=device), None
        xs = xs.contiguous()
        cross = lambda s0, s1, out: self._psi1(xs[s0:s1], sv[s0:s1], out=out)
        for s0, s1, _, wstar in self._star_chunks(xs, budget_bytes, cross=cross):
            dev.sparse_tail(None, wstar, s1 - s0, m, self.gamma, k.sf, 0.0, mean[s0:s1], None, False)
            if scratch is None:
                scratch = torch.empty(max(16, devp.psi2_rows_quad_scratch_bytes(s1 - s0, m, int(xs.shape[1]), q, dt)), dtype=torch.uint8,
                                      device=device)
            devp.psi2_rows_quad(xs[s0:s1], sv[s0:s1], self.z, self._ell_dev, k.sf, c, a, tr=tr[s0:s1], quad=var[s0:s1], scratch=scratch,
                                bad=bad_chunk)
            bad += bad_chunk
        var.sub_(mean * mean).add_((k.sf - tr)[:, None])
        if include_noise:
            var.add_(k.noise)
        count = float(bad.item())
        if count > 0:
            raise ValueError('%d of the test rows have a negative or non-finite variance' % int(count))
        return mean, var

    # ---- what a block with uncertain inputs does not answer ---------------------------------------------------------
    def _ready_for(self, what):
        _not_built('%s()' % what)

    def lml_grad(self, r, want_z=True):
        _not_built('lml_grad() (the analytic gradient of the bound)')

    def fit_layer(self, *args, **kwargs):
        _not_built('fit_layer() (a model layer)')

    def predict_layer(self, *args, **kwargs):
        _not_built('predict_layer() (a model layer)')
