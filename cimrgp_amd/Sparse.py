"""Inducing-point (sparse) GP regression block: FITC and VFE / DTC ("Sparse (inducing-point) GP regression").

With n training inputs X, m inducing inputs Z, covariance k (length-scale l, variance sf), noise s2 and relative jitter eps:

    K_uu + eps sf I = L_u L_u^T              A = K(X, Z) L_u^-T   (n x m)
    q_i = sum_j A_ij^2                       lambda_i = sf - q_i + s2 (FITC)  |  s2 (VFE)
    B = I + A^T Lambda^-1 A = L_B L_B^T      c = A^T Lambda^-1 r,  gamma = L_B^-1 c   (m x q)
    LML = -1/2 n q log 2 pi - 1/2 q sum log lambda_i - q sum log (L_B)_ii - 1/2 sum r_ic^2 / lambda_i + 1/2 |gamma|_F^2
          - 1/2 q sum_i (sf - q_i) / s2      (VFE only: Titsias' trace term)
    A* = K(X*, Z) L_u^-T,  W* = A* L_B^-T    mean* = W* gamma,  var* = sf - sum A*^2 + sum W*^2  (+ s2 with include_noise)

Cost n m^2 flop and n m memory, against n^3 / 3 and n^2 of an exact block.  Every step is a call of the C ABI:
cimrgp_cov_gram, cimrgp_potrf, cimrgp_cov_cross, cimrgp_trsm_rows, cimrgp_sparse_lambda, cimrgp_wsyrk_tn, cimrgp_potrs,
cimrgp_logdet_half and cimrgp_sparse_tail.  torch holds the buffers and adds up the two O(n q) scalars of the LML.
``SparseBlock.lml_grad`` adds the analytic gradient w.r.t. (log sf, log l, log s2) and Z: cimrgp_trsm_rows_lt,
cimrgp_sparse_grad_rows, cimrgp_sparse_grad_combine and cimrgp_cov_pair_grad on the n x m side, torch on the m x m side.
"""
import numpy as np
import torch

from . import device as dev

APPROXIMATIONS = {'fitc': 0, 'vfe': 1, 'dtc': 1}

#: bytes of A* and W* together that ``predict`` works in at a time
PREDICT_BUDGET_BYTES = 1 << 30


class SparseBlock(object):
    """Device-resident state of one inducing-point block: L_u and L_B with their workspaces, and gamma."""

    def __init__(self, x, z, kernel, approximation='fitc', jitter=1e-6):
        """``x`` (n x d), ``z`` (m x d): device tensors in the same units; ``kernel``: an ``RBFKernel`` /
        ``DenseMaternKernel`` with its ``noise`` set."""
        key = str(approximation).lower()
        if key not in APPROXIMATIONS:
            raise ValueError("approximation must be 'fitc' or 'vfe', got %r" % (approximation,))
        if kernel.noise is None or not kernel.noise > 0:
            raise ValueError('a sparse block needs a positive noise variance')
        if not jitter >= 0:
            raise ValueError('jitter must not be negative')
        if x.shape[1] != z.shape[1] or x.dtype != z.dtype:
            raise ValueError('inducing inputs must have the dimension and dtype of the training inputs')
        self.x, self.z = x, z.contiguous()
        self.n, self.m = int(x.shape[0]), int(z.shape[0])
        self.kernel = kernel
        self.approximation = 'fitc' if key == 'fitc' else 'vfe'
        self.mode = APPROXIMATIONS[key]
        self.jitter = float(jitter)
        self.lu = self.ws_u = self.info_u = None
        self.lb = self.ws_b = self.info_b = None
        self.gamma = None
        self._terms = None               # device scalars of the LML

    def _enqueue_fit(self, r):
        """The fit's device calls, nothing read back: (A, w, lambda sums).  A (n x m) is the caller's to free."""
        k, n, m = self.kernel, self.n, self.m
        self.lu = dev.rbf_gram(self.z, k.l, k.sf, self.jitter * k.sf, lower_only=True, cov=k.cov)
        self.ws_u, self.info_u = dev.potrf(self.lu, m)
        a = dev.rbf_cross(self.x, self.z, k.l, k.sf, cov=k.cov)
        dev.trsm_rows(self.lu, m, self.ws_u, a, n)
        _, w, sums = dev.sparse_lambda(a, n, m, k.sf, k.noise, self.mode)
        return a, w, sums

    def _enqueue_solve(self, r, c, w, sums):
        """Factor L_B in place, gamma and the device scalars of the LML; c = A^T W r is overwritten with b = L_B^-T gamma."""
        m, q = self.m, int(r.shape[1])
        self.ws_b, self.info_b = dev.potrf(self.lb, m)
        self.gamma = dev.potrs(self.lb, m, self.ws_b, c, want_z=True)
        half_logdet_b = dev.logdet_half(self.lb, m)
        rwr = (r.double() ** 2 * w.double()[:, None]).sum()
        gg = (self.gamma.double() ** 2).sum()
        self._terms = (sums, half_logdet_b, rwr, gg, q)

    def _raise_if_failed(self, info_u, bad, info_b):
        dev.raise_if_not_pd(info_u)
        if float(bad) > 0:
            raise np.linalg.LinAlgError("sparse GP: %d of the lambda_i = sf - q_i + noise are not positive" % int(bad))
        dev.raise_if_not_pd(info_b)

    def fit(self, r):
        """``r`` (n x q): residual targets on the device.  Nothing is read back but the two ``info`` words and the
        count of non-positive lambda."""
        n, m = self.n, self.m
        r = r.contiguous()
        a, w, sums = self._enqueue_fit(r)
        self.lb, c = dev.wsyrk_tn(a, n, m, w, r, diag_add=1.0)
        del a                                            # n x m: not needed after the fit
        self._enqueue_solve(r, c, w, sums)
        self._raise_if_failed(self.info_u, sums[2].item(), self.info_b)
        return self

    def _lml_from(self, s0, s1, half_logdet_b, rwr, gg, q):
        lml = (-0.5 * self.n * q * np.log(2 * np.pi) - 0.5 * q * s0 - q * float(half_logdet_b)
               - 0.5 * float(rwr) + 0.5 * float(gg))
        if self.mode == 1:
            lml -= 0.5 * q * s1 / self.kernel.noise
        return float(lml)

    def log_marginal_likelihood(self):
        if self._terms is None:
            raise RuntimeError('call fit() before log_marginal_likelihood()')
        sums, half_logdet_b, rwr, gg, q = self._terms
        s = sums.cpu().numpy()
        return self._lml_from(s[0], s[1], half_logdet_b.item(), rwr.item(), gg.item(), q)

    def lml_grad(self, r, want_z=True):
        """Fit on ``r`` (n x q, device) and return ``(lml, dtheta, dZ)``: the objective :meth:`log_marginal_likelihood`
        returns (bit for bit), its gradient w.r.t. (log sf, log l, log noise) as a NumPy (3,) array and, with ``want_z``,
        w.r.t. the inducing inputs as a device tensor (m x d), else None ("Gradients of the sparse
        objective").  The failure rules are :meth:`fit`'s.  A stays alive for the length of the call beside ONE more
        n x m buffer (V, Y, G_A and G_fu in place of one another); one host read-back at the end (the info words, the
        lambda count and the scalars).  g of Matern 1/2 is taken as 0 at r = 0 (an inducing input on a training input or
        on another inducing input, where the objective has a kink): such pairs contribute nothing to dZ."""
        k, n, m = self.kernel, self.n, self.m
        q = int(r.shape[1])
        r = r.contiguous()
        dt, device = self.z.dtype, self.z.device
        a, w, sums = self._enqueue_fit(r)
        self.lb, c = dev.wsyrk_tn(a, n, m, w, r, diag_add=1.0)
        eye = torch.eye(m, dtype=dt, device=device)
        bmat = None
        if self.mode == 1:                               # VFE: A^T diag(t) A = -(q / 2) (B - I), from B before it is factored
            bmat = torch.tril(self.lb[:m, :m])
            bmat = bmat + torch.tril(bmat, -1).t()
        self._enqueue_solve(r, c, w, sums)
        b = c                                            # potrs left B^-1 c = L_B^-T gamma in c
        # the n x m chain, in place in ONE buffer beside A: V = A L_B^-T, Y = V L_B^-1, G_A, G_fu = G_A L_u^-1
        y = torch.empty_like(a)
        y.copy_(a)
        dev.trsm_rows(self.lb, m, self.ws_b, y, n)
        beta, t, gsums = dev.sparse_grad_rows(y, n, m, self.gamma, r, w, self.mode, k.noise)
        dev.trsm_rows_lt(self.lb, m, self.ws_b, y, n)
        dev.sparse_grad_combine(a, y, n, m, beta, b, w, t)
        dev.trsm_rows_lt(self.lu, m, self.ws_u, y, n)
        # the m x m plumbing: B^-1 from the identity, M = b b^T - q (I - B^-1) - 2 A^T diag(t) A, G_uu = -1/2 L_u^-T M L_u^-1
        binv = dev.alloc_matrix(m, m, dt, device)
        binv.zero_()
        binv[:m, :m].fill_diagonal_(1.0)
        dev.trsm_rows(self.lb, m, self.ws_b, binv, m)
        dev.trsm_rows_lt(self.lb, m, self.ws_b, binv, m)
        if self.mode == 0:
            ata, _ = dev.wsyrk_tn(a, n, m, t)
            ata = torch.tril(ata[:m, :m])
            ata = ata + torch.tril(ata, -1).t()
        else:
            ata = (-0.5 * q) * (bmat - eye)
        del a
        mm = b @ b.t() - q * (eye - binv[:m, :m]) - 2.0 * ata
        guu = dev.alloc_matrix(m, m, dt, device)
        guu[:m, :m] = 0.5 * (mm + mm.t())
        dev.trsm_rows_lt(self.lu, m, self.ws_u, guu, m)
        guu[:m, :m] = guu[:m, :m].t().clone()
        dev.trsm_rows_lt(self.lu, m, self.ws_u, guu, m)
        guu[:m, :m] = -0.25 * (guu[:m, :m] + guu[:m, :m].t())
        # sum G o K, sum G o dK/dlog l and dZ: K_fu's pairs, then K_uu's added (G_uu symmetric: scale 2 = -2 x -1)
        psums, dz = dev.cov_pair_grad(self.x, self.z, y, k.l, k.sf, want_db=want_z, cov=k.cov)
        dev.cov_pair_grad(self.z, self.z, guu, k.l, k.sf, scale=2.0, accumulate=True, sums=psums, db=dz, want_db=want_z, cov=k.cov)
        del y
        _, half_logdet_b, rwr, gg, _ = self._terms
        host = torch.cat([self.info_u.double(), self.info_b.double(), sums, half_logdet_b.reshape(1), rwr.reshape(1), gg.reshape(1),
                          gsums, psums, torch.diagonal(mm).double().sum().reshape(1),
                          torch.diagonal(guu[:m, :m]).double().sum().reshape(1)]).cpu().numpy()
        info_u, info_b, s0, s1, bad, hld, rwr_h, gg_h, sum_h, sum_t, gk, gl, tr_m, tr_guu = host
        self._raise_if_failed(info_u, bad, info_b)
        lml = self._lml_from(s0, s1, hld, rwr_h, gg_h, q)
        dsf = 0.5 * tr_m + k.sf * sum_t
        dnoise = k.noise * (sum_h + (0.5 * q / k.noise ** 2 * s1 if self.mode == 1 else 0.0))
        #: the pairwise form of d F / d log sf, which the closed form above must equal (checked by the GPU tests)
        self.grad_check = dict(closed=float(dsf), pairwise=float(gk + self.jitter * k.sf * tr_guu + k.sf * sum_t))
        return lml, np.array([dsf, gl, dnoise]), dz

    def chunk_rows(self, budget_bytes=None):
        """Test rows per pass of ``predict``: A* and W* (pitch padded_ld(m)) within ``budget_bytes``, a multiple of 256."""
        budget = PREDICT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
        per_row = 2 * dev.padded_ld(self.m) * self.z.element_size()
        return max(256, budget // per_row // 256 * 256)

    def predict(self, xs, mean=None, var=None, include_noise=False, budget_bytes=None):
        """Predictive mean into ``mean`` (ns x q) and variance into ``var`` (ns,) at ``xs`` (ns x d, device); either may
        be None.  Works in chunks of ``chunk_rows(budget_bytes)`` test rows: a row's result does not depend on the
        chunking."""
        if self.gamma is None:
            raise RuntimeError('call fit() before predict()')
        k, m = self.kernel, self.m
        ns = int(xs.shape[0])
        step = self.chunk_rows(budget_bytes)
        extra = k.noise if include_noise else 0.0
        astar = wstar = None
        for s0 in range(0, ns, step):
            s1 = min(ns, s0 + step)
            rows = s1 - s0
            if astar is None:
                astar = dev.alloc_matrix(min(step, ns), m, xs.dtype, xs.device)
                wstar = torch.empty_like(astar)
            dev.rbf_cross(xs[s0:s1], self.z, k.l, k.sf, out=astar, cov=k.cov)
            dev.trsm_rows(self.lu, m, self.ws_u, astar, rows)
            wstar[:rows].copy_(astar[:rows])
            dev.trsm_rows(self.lb, m, self.ws_b, wstar, rows)
            dev.sparse_tail(astar if var is not None else None, wstar, rows, m, self.gamma if mean is not None else None, k.sf,
                            extra, None if mean is None else mean[s0:s1], None if var is None else var[s0:s1])
        return mean, var
