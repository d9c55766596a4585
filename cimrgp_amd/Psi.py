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


class UncertainInputBlock(SparseBlock):
    """Device-resident state of one sparse block whose training inputs are Gaussians: L_u, L_B, gamma as a
    :class:`~cimrgp_amd.Sparse.SparseBlock` keeps them ('vfe'), built from the psi statistics."""

    def __init__(self, x_mean, x_var, z, kernel, jitter=1e-6, lengthscales=None):
        """``x_mean`` (n x d), ``z`` (m x d): float64 device tensors in the same units; ``kernel``: an ``RBFKernel`` with its
        ``noise`` set; ``lengthscales``: as for ``SparseBlock`` (ARD; ``kernel.l`` must then be 1.0).  ``x_var``: the
        variances of the inputs in the squared units of ``x_mean`` -- a scalar or a (d,) vector (every row has that
        variance: the shared-variance route, checked non-negative and finite here) or an (n, d) device tensor (the psi
        kernels; a negative or non-finite entry is found by the device and raises ValueError in :meth:`fit`).  A Matern
        covariance has no closed-form psi statistics and is refused, as are float32 blocks."""
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
        self.bad = self._f_terms = None

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

    # ---- prediction ---------------------------------------------------------------------------------------------
    def predict(self, xs, mean=None, var=None, include_noise=False, budget_bytes=None, xs_var=None):
        """``SparseBlock.predict`` at exact test inputs.  ``xs_var`` (a scalar, a (d,) vector or an (ns, d) device
        tensor): the test inputs are Gaussians too and the mean is E_x* [k(x*, Z)] K_uu^-1 .. = Psi1* L_u^-T L_B^-T gamma;
        the variance at uncertain test inputs is not built."""
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

    # ---- what a block with uncertain inputs does not answer ---------------------------------------------------------
    def _ready_for(self, what):
        _not_built('%s()' % what)

    def lml_grad(self, r, want_z=True):
        _not_built('lml_grad() (the analytic gradient of the bound)')

    def fit_layer(self, *args, **kwargs):
        _not_built('fit_layer() (a model layer)')

    def predict_layer(self, *args, **kwargs):
        _not_built('predict_layer() (a model layer)')
