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

    def fit(self, r):
        """``r`` (n x q): residual targets on the device.  Nothing is read back but the two ``info`` words and the
        count of non-positive lambda."""
        k, n, m = self.kernel, self.n, self.m
        q = int(r.shape[1])
        r = r.contiguous()
        self.lu = dev.rbf_gram(self.z, k.l, k.sf, self.jitter * k.sf, lower_only=True, cov=k.cov)
        self.ws_u, self.info_u = dev.potrf(self.lu, m)
        a = dev.rbf_cross(self.x, self.z, k.l, k.sf, cov=k.cov)
        dev.trsm_rows(self.lu, m, self.ws_u, a, n)
        _, w, sums = dev.sparse_lambda(a, n, m, k.sf, k.noise, self.mode)
        self.lb, c = dev.wsyrk_tn(a, n, m, w, r, diag_add=1.0)
        del a                                            # n x m: not needed after the fit
        self.ws_b, self.info_b = dev.potrf(self.lb, m)
        self.gamma = dev.potrs(self.lb, m, self.ws_b, c, want_z=True)
        half_logdet_b = dev.logdet_half(self.lb, m)
        rwr = (r.double() ** 2 * w.double()[:, None]).sum()
        gg = (self.gamma.double() ** 2).sum()
        self._terms = (sums, half_logdet_b, rwr, gg, q)
        dev.raise_if_not_pd(self.info_u)
        if float(sums[2].item()) > 0:
            raise np.linalg.LinAlgError("sparse GP: %d of the lambda_i = sf - q_i + noise are not positive" % int(sums[2].item()))
        dev.raise_if_not_pd(self.info_b)
        return self

    def log_marginal_likelihood(self):
        if self._terms is None:
            raise RuntimeError('call fit() before log_marginal_likelihood()')
        sums, half_logdet_b, rwr, gg, q = self._terms
        s = sums.cpu().numpy()
        lml = (-0.5 * self.n * q * np.log(2 * np.pi) - 0.5 * q * s[0] - q * float(half_logdet_b.item())
               - 0.5 * float(rwr.item()) + 0.5 * float(gg.item()))
        if self.mode == 1:
            lml -= 0.5 * q * s[1] / self.kernel.noise
        return float(lml)

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
