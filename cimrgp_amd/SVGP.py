"""Variational sparse GP regression block with a non-conjugate likelihood ("Variational sparse GP with a
Student-t likelihood"): GPy's ``SVGP`` with a Student-t (or Gaussian) likelihood, full batch, whitened.

With n training inputs X, m inducing inputs Z, the covariance k of a :class:`Sparse.BlockCovariance` (plain, ARD, linear),
a fixed white variance added to k(x, x) and to the diagonal of K_uu, and per output column c the variational distribution
q(v_c) = N(mu_c, (P_c P_c^T)^-1) of the whitened inducing values u = L_u v:

    K_uu + (eps sf + white) I = L_u L_u^T      A = K(X, Z) L_u^-T                    cov.gram, cimrgp_potrf, cov.cross, cimrgp_trsm_rows
    W_c = A P_c^-T,  gamma_c = P_c^T mu_c      m_ic = W_c,i gamma_c                  cimrgp_trsm_rows
    v_ic = kdiag_i - sum_j A_ij^2 + sum_j W_c,ij^2,   kdiag_i = sf + sum_e u_e x_ie^2 + white
    E_ic = pi^-1/2 sum_h omega_h log p(y_ic | m_ic + sqrt(2 v_ic) x_h)               cimrgp_svgp_rows (H Gauss-Hermite nodes)
    KL_c = 1/2 (|P_c^-1|_F^2 + mu_c^T mu_c - m + 2 sum log diag P_c)
    F = sum_c [sum_i E_ic - KL_c]

The gradient follows from the rows' g1 = dE/dm, g2 = dE/dv: N_c = A^T diag(g2_c) A and a_c = A^T g1_c come from ONE pass
over A (cimrgp_svgp_moments), dF/dA from cimrgp_sparse_grad_combine, and the hyper-parameters' share through the pair
contractions of the sparse objective (``BlockCovariance.pair_grad``).  All n x m work is a call of the C ABI; torch holds
the buffers and does the m x m algebra (:func:`column_terms`, :func:`kuu_weight`, which run on any device and are checked
on the CPU against autograd).  The row solves take P_c through ``cimrgp_potrf`` of P_c P_c^T, which gives the factor back
together with the workspace the solves need."""
import numpy as np
import torch

from . import _lib
from . import device as dev
from . import device_svgp as devs
from .Sparse import BlockCovariance, read_back, rows_within, star_rows

LIKELIHOODS = {'gaussian': _lib.LIK_GAUSSIAN, 'student_t': _lib.LIK_STUDENT_T}

#: Gauss-Hermite nodes of the expectation
NODES = 20


def hermite_nodes(nodes=NODES):
    """The ``nodes`` Gauss-Hermite nodes, then their weights: float64 (2 nodes,), as cimrgp_svgp_rows takes them."""
    x, w = np.polynomial.hermite.hermgauss(int(nodes))
    return np.concatenate([x, w])


def column_terms(p, mu, nmat, avec):
    """One output column's m x m share, torch on any device: from P (m x m lower), mu (m,), N = A^T diag(g2) A (m x m,
    symmetric) and a = A^T g1 (m,), returns (dF/dmu, dF/dP (lower), A^T (dF/dA) (m x m), KL)."""
    m = p.shape[0]
    eye = torch.eye(m, dtype=p.dtype, device=p.device)
    pinv = torch.linalg.solve_triangular(p, eye, upper=False)
    s = pinv.t() @ pinv
    dmu = avec - mu
    dp = torch.tril(-2.0 * s @ nmat @ pinv.t() + s @ pinv.t()) - torch.diag(1.0 / torch.diagonal(p))
    ata = torch.outer(avec, mu) + 2.0 * nmat @ (s - eye)
    kl = 0.5 * ((pinv * pinv).sum() + mu @ mu - m + 2.0 * torch.log(torch.diagonal(p)).sum())
    return dmu, dp, ata, kl


def kuu_weight(lu, ata):
    """G_uu = dF / dK_uu (symmetric, m x m) through A = K_fu L_u^-T alone, from L_u (lower) and A^T Abar = ``ata``, Abar =
    dF/dA: Lbar = -tril(L_u^-T Abar^T A), then the Cholesky factor's backward rule G = L^-T Phi(L^T Lbar) L^-1, Phi =
    the lower triangle with its diagonal halved, symmetrised."""
    lbar = -torch.tril(torch.linalg.solve_triangular(lu.t(), ata.t(), upper=True))
    phi = torch.tril(lu.t() @ lbar)
    phi = phi - 0.5 * torch.diag(torch.diagonal(phi))
    g = torch.linalg.solve_triangular(lu.t(), phi, upper=True)
    g = torch.linalg.solve_triangular(lu.t(), g.t(), upper=True).t()
    return 0.5 * (g + g.t())


class SVGPBlock(object):
    """Device-resident state of one variational block: L_u with its workspace and, after :meth:`set_posterior`, every
    output's factor P_c with its workspace and gamma_c."""

    def __init__(self, x, z, kernel, likelihood='student_t', deg_free=3., scale=0.01, white=0.01, jitter=1e-6, lengthscales=None,
                 linear=None, nodes=NODES):
        """``x`` (n x d), ``z`` (m x d): device tensors in the same units; ``kernel``: an ``RBFKernel`` / ``DenseMaternKernel``
        (its ``noise`` is not used: the likelihood has its own ``scale`` s2).  ``likelihood``: 'student_t' with ``deg_free``
        degrees of freedom, or 'gaussian'.  ``white``: a fixed variance added to k(x, x) and to the diagonal of K_uu, not to
        K(X, Z) (GPy's ``White``).  ``lengthscales``, ``linear``: as :class:`Sparse.SparseBlock` takes them."""
        key = str(likelihood).lower()
        if key not in LIKELIHOODS:
            raise ValueError("likelihood must be 'student_t' or 'gaussian', got %r" % (likelihood,))
        if not scale > 0:
            raise ValueError("the likelihood's scale must be positive")
        if key == 'student_t' and not deg_free > 0:
            raise ValueError('deg_free must be positive')
        if not white >= 0 or not jitter >= 0:
            raise ValueError('white and jitter must not be negative')
        if not 1 <= int(nodes) <= 64:
            raise ValueError('nodes must be in [1, 64]')
        if x.shape[1] != z.shape[1] or x.dtype != z.dtype:
            raise ValueError('inducing inputs must have the dimension and dtype of the training inputs')
        if x.dtype != torch.float64:
            raise TypeError('a variational sparse block in float32 is not yet supported')
        self.x, self.z = x, z.contiguous()
        self.cov = BlockCovariance(kernel, x, lengthscales, linear)
        self.lengthscales, self.linear = self.cov.lengthscales, self.cov.linear
        self._xs, self._zs = self.cov.inputs(self.x), self.cov.inputs(self.z)
        self.n, self.m = int(x.shape[0]), int(z.shape[0])
        self.kernel, self.likelihood, self.lik = kernel, key, LIKELIHOODS[key]
        self.deg_free, self.scale, self.white, self.jitter = float(deg_free), float(scale), float(white), float(jitter)
        self.nodes = torch.as_tensor(hermite_nodes(nodes)).to(x.device)
        self.lu = self.ws_u = self.info_u = None
        self._columns = None             # per output: (P_c's buffer, its workspace, its info, gamma_c)

    # ---- the shared steps ----
    def _diag_add(self):
        return self.jitter * self.kernel.sf + self.white

    def _enqueue_lu(self):
        self.lu = self.cov.gram(self._zs, self._diag_add())
        self.ws_u, self.info_u = dev.potrf(self.lu, self.m)

    def _kdiag(self, xs):
        """k(x_i, x_i) + white of scaled inputs ``xs``, of their dtype."""
        kd = torch.full((int(xs.shape[0]),), self.kernel.sf + self.white, dtype=torch.float64, device=xs.device)
        if self.cov.lin is not None:
            kd = kd + self.cov.linear_diag(xs)
        return kd.to(xs.dtype)

    def _enqueue_column(self, mu_c, p_c):
        """(P_c's buffer, workspace, info, gamma_c): the factor of P_c P_c^T, which is P_c, with the workspace cimrgp_potrf
        leaves for the row solves."""
        m = self.m
        pb = dev.alloc_matrix(m, m, p_c.dtype, p_c.device)
        pb[:m, :m] = p_c @ p_c.t()
        ws_p, info_p = dev.potrf(pb, m)
        return pb, ws_p, info_p, (p_c.t() @ mu_c).contiguous()

    def _check_posterior(self, mu, p, q=None):
        m = self.m
        if mu.dim() != 2 or p.dim() != 3 or tuple(p.shape) != (int(mu.shape[0]), m, m) or int(mu.shape[1]) != m:
            raise ValueError('mu must be (q, m) and P (q, m, m)')
        if q is not None and int(mu.shape[0]) != q:
            raise ValueError('mu and P must have one entry per output column')
        if mu.dtype != self.x.dtype or p.dtype != self.x.dtype or mu.device != self.x.device or p.device != self.x.device:
            raise ValueError("mu and P must be device tensors of the block's dtype")
        if not 1 <= int(mu.shape[0]) <= 8:
            raise ValueError('the number of outputs must be in [1, 8]')

    # ---- objective and gradient ----
    def elbo_grad(self, y, mu, p):
        """``(F, dtheta, dmu, dP)`` at q(v_c) = N(mu[c], (P[c] P[c]^T)^-1): ``y`` (n x q), ``mu`` (q, m), ``p`` (q, m, m; the
        lower triangle is P_c, with a positive diagonal) on the device.  dtheta is a NumPy array w.r.t. (log sf, log l (1, or d
        under ARD), log s2, and with a linear term log v_1 .. log v_d); dmu (q, m) and dP (q, m, m, lower) are device tensors.
        Z is fixed.  A, and one more n x m buffer that serves the outputs in turn, stay alive for the call; one host
        read-back at its end.  Raises LinAlgError if K_uu + (eps sf + white) I or a P_c P_c^T is not positive definite, or
        a latent variance v_ic is not positive."""
        n, m, k = self.n, self.m, self.kernel
        q = int(y.shape[1])
        self._check_posterior(mu, p, q)
        if int(y.shape[0]) != n or y.dtype != self.x.dtype:
            raise ValueError("y must be (n x q) of the block's dtype")
        self._enqueue_lu()
        a = self.cov.cross(self._xs, self._zs)
        dev.trsm_rows(self.lu, m, self.ws_u, a, n)
        kdiag = self._kdiag(self._xs)
        work = torch.empty_like(a)
        lu = torch.tril(self.lu[:m, :m])
        t = torch.zeros(n, dtype=a.dtype, device=a.device)
        ata = torch.zeros((m, m), dtype=a.dtype, device=a.device)
        sums = torch.zeros(3, dtype=torch.float64, device=a.device)
        kl = torch.zeros((), dtype=torch.float64, device=a.device)
        infos, dmu, dp, pair = [], torch.empty_like(mu), torch.empty_like(p), None
        for c in range(q):
            mu_c, p_c = mu[c], torch.tril(p[c])
            pb, ws_p, info_p, gamma_c = self._enqueue_column(mu_c, p_c)
            infos.append(info_p)
            work.copy_(a)
            dev.trsm_rows(pb, m, ws_p, work, n)                          # W_c = A P_c^-T
            rows = devs.svgp_rows(a, work, n, m, gamma_c, kdiag, y[:, c], self.nodes, self.lik, self.scale, self.deg_free,
                                 want=("g1", "g2", "sums"))
            g1, g2 = rows["g1"], rows["g2"]
            nlow, avec = devs.svgp_moments(a, n, m, g2, g1[:, None])
            nlow = torch.tril(nlow[:m, :m])
            dmu[c], dp[c], ata_c, kl_c = column_terms(p_c, mu_c, nlow + torch.tril(nlow, -1).t(), avec[:, 0])
            dev.trsm_rows_lt(pb, m, ws_p, work, n)                       # Y_c = W_c P_c^-1
            dev.sparse_grad_combine(a, work, n, m, g1[:, None], mu_c[:, None].contiguous(), -2.0 * g2, g2)
            dev.trsm_rows_lt(self.lu, m, self.ws_u, work, n)             # this output's share of G_fu
            pair = self.cov.pair_grad(self._xs, self._zs, work, False, into=pair)
            t, ata, sums, kl = t + g2, ata + ata_c, sums + rows["sums"], kl + kl_c
        del a, work
        guu = dev.alloc_matrix(m, m, lu.dtype, lu.device)
        guu.zero_()
        guu[:m, :m] = kuu_weight(lu, ata)
        psums, lsums, _ = self.cov.pair_grad(self._zs, self._zs, guu, False, into=pair)
        h = read_back(dict(info_u=self.info_u, info_p=torch.stack([i.reshape(()) for i in infos]).max(), kl=kl,
                           tr_guu=torch.diagonal(guu[:m, :m]).double().sum(), sum_t=t.double().sum()),
                      dict(sums=sums, psums=psums, lsums=lsums, tx2=self.cov.diag_grad(t, self._xs)))
        dev.raise_if_not_pd(h['info_u'])
        dev.raise_if_not_pd(h['info_p'])
        if h['sums'][2] > 0:
            raise np.linalg.LinAlgError("variational sparse GP: %d of the latent variances v_i are not positive" % int(h['sums'][2]))
        gk, gl = h['psums'][0], h['psums'][1:]
        dsf = gk + self.jitter * k.sf * h['tr_guu'] + k.sf * h['sum_t']
        parts = [[dsf], gl, [h['sums'][1]]]
        if self.cov.u is not None:
            parts.append(self.cov.u * (h['lsums'] + h['tx2']))
        return float(h['sums'][0] - h['kl']), np.concatenate(parts), dmu, dp

    # ---- prediction ----
    def set_posterior(self, mu, p):
        """Keep q(v_c) = N(mu[c], (P[c] P[c]^T)^-1) for :meth:`predict`: L_u, and per output the factor P_c with its
        workspace and gamma_c.  One host read: the info words."""
        self._check_posterior(mu, p)
        self._enqueue_lu()
        self._columns = [self._enqueue_column(mu[c], torch.tril(p[c])) for c in range(int(mu.shape[0]))]
        dev.raise_if_not_pd(torch.stack([self.info_u.reshape(())] + [col[2].reshape(()) for col in self._columns]).max())
        return self

    def chunk_rows(self, budget_bytes=None):
        """Test rows per pass of :meth:`predict`, a multiple of 256: A* and W* within ``budget_bytes``."""
        return rows_within(self.z, budget_bytes)

    def predict(self, xs, mean=None, var=None, budget_bytes=None):
        """The latent f at ``xs`` (ns x d, device): mean into ``mean`` (ns x q), variance per output into ``var`` (ns x q);
        either may be None.  Chunks of ``chunk_rows(budget_bytes)`` test rows (``Sparse.star_rows``: A* = K(X*, Z) L_u^-T,
        which every output then takes through its own P_c): a row's result does not depend on the chunking."""
        if self._columns is None:
            raise RuntimeError('call set_posterior() before predict()')
        m, k = self.m, self.kernel
        for s0, s1, astar, wstar in star_rows(self.cov, self._zs, self.lu, self.ws_u, m, xs, self.chunk_rows(budget_bytes)):
            rows = s1 - s0
            seed = None if self.cov.lin is None else self.cov.linear_diag(self.cov.inputs(xs[s0:s1])).to(xs.dtype)
            for c, (pb, ws_p, _, gamma_c) in enumerate(self._columns):
                wstar[:rows].copy_(astar[:rows])
                dev.trsm_rows(pb, m, ws_p, wstar, rows)
                # with a linear term the tail adds onto k(x*, x*)'s linear share (and onto a zeroed mean)
                mean_c = None if mean is None else torch.zeros((rows, 1), dtype=xs.dtype, device=xs.device)
                var_c = None if var is None else (torch.empty(rows, dtype=xs.dtype, device=xs.device) if seed is None else seed.clone())
                dev.sparse_tail(astar if var is not None else None, wstar, rows, m, gamma_c[:, None] if mean is not None else None,
                                k.sf, self.white, mean_c, var_c, accumulate=seed is not None)
                if mean is not None:
                    mean[s0:s1, c] = mean_c[:, 0]
                if var is not None:
                    var[s0:s1, c] = var_c
        return mean, var
