"""Inducing-point (sparse) GP regression block: FITC and VFE / DTC ("Sparse (inducing-point) GP regression").

With n training inputs X, m inducing inputs Z, covariance k (length-scale l, variance sf), noise s2 and relative jitter eps:

    K_uu + eps sf I = L_u L_u^T              A = K(X, Z) L_u^-T   (n x m)
    q_i = sum_j A_ij^2                       lambda_i = k(x_i, x_i) - q_i + s2 (FITC)  |  s2 (VFE)
    B = I + A^T Lambda^-1 A = L_B L_B^T      c = A^T Lambda^-1 r,  gamma = L_B^-1 c   (m x q)
    LML = -1/2 n q log 2 pi - 1/2 q sum log lambda_i - q sum log (L_B)_ii - 1/2 sum r_ic^2 / lambda_i + 1/2 |gamma|_F^2
          - 1/2 q sum_i (k(x_i, x_i) - q_i) / s2      (VFE only: Titsias' trace term)
    A* = K(X*, Z) L_u^-T,  W* = A* L_B^-T    mean* = W* gamma,  var* = k(x*, x*) - sum A*^2 + sum W*^2  (+ s2 with include_noise)

Cost n m^2 flop and n m memory, against n^3 / 3 and n^2 of an exact block.  Every step is a call of the C ABI; torch holds
the buffers, adds up the two O(n q) scalars of the LML and does the m x m plumbing of the gradient.

Two classes share the work.  :class:`BlockCovariance` is the covariance k as the device calls take it, and the only place
that knows which of its arms a block is in:

    plain         k = k_cov at the kernel's l                    cimrgp_cov_gram / _cross, cimrgp_sparse_lambda, cimrgp_cov_pair_grad
    ARD           ``lengthscales=``: k_cov at l = 1 on x / l     the same calls on scaled inputs, cimrgp_cov_pair_grad_ard
    linear        ``linear=``: k_cov + sum_e v_e x_e x'_e        cimrgp_cov_gram_lin / _cross_lin, cimrgp_sparse_lambda_kd,
                                                                 cimrgp_cov_pair_grad_lin (include/cimrgp_sparse_linear.h)
    ARD + linear  both: the weights on x / l are u = v l^2       the _lin calls with ``ard``

It scales inputs into the block's units (``inputs``), builds K_uu and K(., Z) (``gram``, ``cross``), gives k(x, x) its
linear share (``linear_diag``, ``lambda_pass``, ``seed_tail``), contracts a weight matrix with dK (``pair_grad``) and takes
gradients back to the caller's units (``chain_rule``).  DESIGN.md, "ARD length-scales for the sparse GP" and "A linear term
for the sparse GP", has the mathematics of the arms.

:class:`SparseBlock` is the algebra above, written once over that object: ``fit`` / ``predict``
(cimrgp_potrf, cimrgp_trsm_rows, cimrgp_wsyrk_tn, cimrgp_potrs, cimrgp_logdet_half, cimrgp_sparse_tail), ``lml_grad`` (the
analytic gradient w.r.t. the hyper-parameters and Z: cimrgp_trsm_rows_lt, cimrgp_sparse_grad_rows,
cimrgp_sparse_grad_combine on the n x m side; DESIGN.md, "Gradients of the sparse objective"), and ``predict_grad``,
``loo`` and ``joint`` ("Posterior queries of the sparse GP": cimrgp_cov_cross_grad, cimrgp_sparse_tail_grad,
cimrgp_sparse_loo, cimrgp_sparse_joint_cov), which are not built for a covariance with a linear term.
:class:`SparsePosterior` makes such blocks a layer of ``MultiResolutionGaussianProcess`` (``KernelClass.SparseKernel``;
DESIGN.md, "Sparse layers in the multiresolution model"): ``SparseBlock.fit_layer`` / ``predict_layer`` take the noise and
the bias from device scalars (cimrgp_sparse_lambda_dev, cimrgp_sparse_tail_dev) and read nothing back; a layer's block is
plain, and answers none of the posterior queries.
"""
import numpy as np
import torch

from . import device as dev
from . import device_linear as devl
from .Hyper import scaled, sum_block_objectives, unit_lengthscale
from .Posteriors import DensePosterior, NOISE_FRACTION, NOISE_FLOOR, _Fanout, block_targets, joint_blocks

APPROXIMATIONS = {'fitc': 0, 'vfe': 1, 'dtc': 1}

#: bytes of A* and W* together that ``predict`` works in at a time
PREDICT_BUDGET_BYTES = 1 << 30


def read_back(scalars, vectors):
    """ONE copy to the host of named device tensors: ``scalars`` (name -> a tensor of one element) come back as floats,
    ``vectors`` (name -> a 1-d tensor, or None: left out) as float64 arrays of their own length, in one dict."""
    vectors = {name: t for name, t in vectors.items() if t is not None}
    parts = [t.double().reshape(-1) for t in (*scalars.values(), *vectors.values())]
    ends, host = np.cumsum([p.numel() for p in parts]), torch.cat(parts).cpu().numpy()      # the ends first: before the wait
    return {k: float(host[e - 1]) if k in scalars else host[e - p.numel():e] for k, p, e in zip((*scalars, *vectors), parts, ends)}


def rows_within(z, budget_bytes=None, slabs=1):
    """Test rows per pass over the inducing inputs ``z`` (m x d), a multiple of 256: ``slabs`` row blocks of A* and as many
    of W* (pitch padded_ld(m)) per test row within ``budget_bytes`` (None: PREDICT_BUDGET_BYTES)."""
    budget = PREDICT_BUDGET_BYTES if budget_bytes is None else int(budget_bytes)
    return max(256, budget // (2 * slabs * dev.padded_ld(int(z.shape[0])) * z.element_size()) // 256 * 256)


def star_rows(cov, zs, lu, ws_u, m, xs, step, cross=None):
    """(s0, s1, A*, W*) of every chunk of ``step`` rows of the test inputs ``xs``: A* = K(xs[s0:s1], Z) L_u^-T in the first
    of two work buffers, allocated at the first chunk and overwritten by the next; W* is the second, left to the caller
    (``SparseBlock``: A* L_B^-T; ``SVGP.SVGPBlock``: A* P_c^-T per output).  ``cov``: the block's BlockCovariance, ``zs``
    its scaled inducing inputs, ``lu`` / ``ws_u``: L_u with its workspace.  ``cross(s0, s1, out)``: what fills ``out`` with
    the chunk's rows in place of K(xs[s0:s1], Z) (``Psi.UncertainInputBlock``: Psi1 of uncertain test inputs)."""
    ns = int(xs.shape[0])
    astar = wstar = None
    for s0 in range(0, ns, step):
        s1 = min(ns, s0 + step)
        if astar is None:
            astar = dev.alloc_matrix(min(step, ns), m, xs.dtype, xs.device)
            wstar = torch.empty_like(astar)
        if cross is None:
            cov.cross(cov.inputs(xs[s0:s1]), zs, out=astar)
        else:
            cross(s0, s1, astar)
        dev.trsm_rows(lu, m, ws_u, astar, s1 - s0)
        yield s0, s1, astar, wstar


class BlockCovariance(object):
    """The covariance of a sparse block as the device calls take it (module docstring): ``kernel``'s values, ``scale`` =
    1 / l on the device under ARD (else None), and under a linear term the weights ``u`` = v l^2 on the host and ``lin``,
    the same as a device float64 (d,) tensor (else None).  ``lengthscales`` and ``linear`` keep the caller's values."""

    def __init__(self, kernel, x, lengthscales=None, linear=None, device_noise=False):
        d = int(x.shape[1])
        self.kernel = kernel
        self.lengthscales = self.scale = self.linear = self.u = self.lin = None
        if lengthscales is not None:
            ls = np.asarray(lengthscales, dtype=np.float64)
            if ls.shape != (d,) or not (np.isfinite(ls).all() and (ls > 0).all()):
                raise ValueError('lengthscales must be %d positive numbers, one per input dimension' % d)
            if kernel.l != 1.0:
                raise ValueError('with lengthscales the kernel must have l = 1.0, got %r' % (kernel.l,))
            if device_noise:
                raise ValueError('lengthscales are not available to a model layer (device_noise=True)')
            self.lengthscales = ls.copy()
            self.scale = torch.as_tensor(1.0 / ls, dtype=x.dtype, device=x.device)       # as Hyper.unit_lengthscale forms it
        if linear is not None:
            v = np.asarray(linear, dtype=np.float64)
            if v.shape != (d,) or not (np.isfinite(v).all() and (v > 0).all()):
                raise ValueError('linear must be %d positive variances, one per input dimension' % d)
            if device_noise:
                raise ValueError('a linear term is not available to a model layer (device_noise=True)')
            self.linear = v.copy()
            self.u = v if self.lengthscales is None else v * self.lengthscales ** 2
            self.lin = torch.as_tensor(self.u, dtype=torch.float64).to(x.device)

    def inputs(self, x):
        """``x`` in the block's units: ``x`` itself, or x / l under ARD.  Training, inducing and test inputs all pass here."""
        return x if self.scale is None else scaled(x, self.scale)

    def gram(self, zs, diag_add):
        """The lower triangle of K(zs, zs) + diag_add I in a new padded buffer."""
        k = self.kernel
        if self.lin is None:
            return dev.rbf_gram(zs, k.l, k.sf, diag_add, lower_only=True, cov=k.cov)
        return devl.cov_gram_lin(zs, k.l, k.sf, self.lin, diag_add, lower_only=True, cov=k.cov)

    def cross(self, xs, zs, out=None):
        """K(xs, zs), into ``out`` or a new padded buffer."""
        k = self.kernel
        if self.lin is None:
            return dev.rbf_cross(xs, zs, k.l, k.sf, out=out, cov=k.cov)
        return devl.cov_cross_lin(xs, zs, k.l, k.sf, self.lin, out=out, cov=k.cov)

    def linear_diag(self, xs):
        """sum_e u_e xs_ie^2 of scaled inputs ``xs``: the linear term's share of k(x_i, x_i), FP64 (O(n d) torch arithmetic)."""
        return (xs.double() ** 2 * self.lin).sum(dim=1)

    def lambda_pass(self, a, n, m, xs, mode, noise_dev=None):
        """(lambda, w = 1 / lambda, sums) of A = ``a`` (n x m) over the scaled inputs ``xs``, from k(x_i, x_i) = sf (+ the
        linear share).  ``noise_dev``: the noise variance as a device scalar, in place of ``kernel.noise``."""
        k = self.kernel
        if self.lin is not None:
            kdiag = (k.sf + self.linear_diag(xs)).to(xs.dtype)
            return devl.sparse_lambda_kd(a, n, m, kdiag, k.noise, mode)
        if noise_dev is not None:
            return dev.sparse_lambda_dev(a, n, m, k.sf, noise_dev, mode)
        return dev.sparse_lambda(a, n, m, k.sf, k.noise, mode)

    def seed_tail(self, xs, mean, var):
        """What cimrgp_sparse_tail starts from at the test inputs ``xs`` (the caller's units).  k(x*, x*) the constant sf:
        nothing, the tail overwrites.  With a linear term, k(x*, x*) = sf + sum_e u_e x*_e^2: ``mean`` is zeroed, ``var``
        takes the linear share, and the tail adds onto them.  Returns the tail's ``accumulate``."""
        if self.lin is None:
            return False
        if mean is not None:
            mean.zero_()
        if var is not None:
            var.copy_(self.linear_diag(self.inputs(xs)))
        return True

    def pair_grad(self, xa, xb, g, want_db, scale=1.0, into=None):
        """``(sums, lsums, db)`` of the weight matrix ``g`` over the pairs (xa_i, xb_j): sums = [sum G o K_cov, sum G o
        dK_cov/dlog l (ARD: one per length-scale)], lsums_e = sum G o dK/du_e (None without a linear term), db = scale
        dF/dxb (None unless ``want_db``).  ``into``: an earlier call's result, which this call adds to."""
        k = self.kernel
        sums, lsums, db = into or (None, None, None)
        kw = dict(scale=scale, accumulate=into is not None, sums=sums, db=db, want_db=want_db, cov=k.cov)
        if self.lin is not None:
            return devl.cov_pair_grad_lin(xa, xb, g, k.l, k.sf, self.lin, ard=self.scale is not None, lsums=lsums, **kw)
        sums, db = (dev.cov_pair_grad if self.scale is None else dev.cov_pair_grad_ard)(xa, xb, g, k.l, k.sf, **kw)
        return sums, None, db

    def diag_grad(self, t, xs):
        """sum_i t_i xs_ie^2 (FP64, (d,)): the share of k(x_i, x_i) in dF / du_e, t_i = dF / dk_ii; None without a linear term."""
        return None if self.lin is None else (t.double()[:, None] * xs.double() ** 2).sum(dim=0)

    def chain_rule(self, dz=None, mean_grad=None, var_grad=None):
        """Gradients w.r.t. inputs in the block's units, taken to the caller's: d / dx_e = (d / d(x_e / l_e)) / l_e.
        ``dz`` (m x d) is returned (a new tensor under ARD); ``mean_grad`` (ns, d, q) and ``var_grad`` (ns, d) change in place."""
        if self.scale is None:
            return dz
        if mean_grad is not None:
            mean_grad.mul_(self.scale[None, :, None])
        if var_grad is not None:
            var_grad.mul_(self.scale[None, :])
        return None if dz is None else dz * self.scale


class SparseBlock(object):
    """Device-resident state of one inducing-point block: L_u and L_B with their workspaces, and gamma."""

    def __init__(self, x, z, kernel, approximation='fitc', jitter=1e-6, device_noise=False, lengthscales=None, linear=None):
        """``x`` (n x d), ``z`` (m x d): device tensors in the same units; ``kernel``: an ``RBFKernel`` /
        ``DenseMaternKernel`` with its ``noise`` set.  ``device_noise``: the block is a model layer's, fitted by
        :meth:`fit_layer` with its noise variance in a device scalar; ``kernel.noise`` may then be None.
        ``lengthscales``: a (d,) array of positive length-scales, one per input dimension (ARD), in the units of ``x``;
        ``kernel.l`` must then be 1.0, as ``GP_RBF(ARD=True)`` builds its kernel.  The block computes on x / l and z / l;
        ``x``, ``z``, the test inputs of :meth:`predict` and the dZ of :meth:`lml_grad` stay in the caller's units.
        ``linear``: a (d,) array of positive variances v_e in the units of ``x``: the covariance is k_cov(x, x') +
        sum_e v_e x_e x'_e (GPy's ``Linear(d, ARD=True)`` added to the kernel); the jitter stays ``jitter * sf``.  On the
        scaled inputs the same term has the weights u_e = v_e l_e^2, which ``cov`` (a :class:`BlockCovariance`) forms;
        callers speak in v.  None: no such term."""
        key = str(approximation).lower()
        if key not in APPROXIMATIONS:
            raise ValueError("approximation must be 'fitc' or 'vfe', got %r" % (approximation,))
        if not device_noise and (kernel.noise is None or not kernel.noise > 0):
            raise ValueError('a sparse block needs a positive noise variance')
        if not jitter >= 0:
            raise ValueError('jitter must not be negative')
        if x.shape[1] != z.shape[1] or x.dtype != z.dtype:
            raise ValueError('inducing inputs must have the dimension and dtype of the training inputs')
        self.x, self.z = x, z.contiguous()
        self.cov = BlockCovariance(kernel, x, lengthscales, linear, device_noise)
        self.lengthscales, self.linear = self.cov.lengthscales, self.cov.linear
        self._xs, self._zs = self.cov.inputs(self.x), self.cov.inputs(self.z)        # what the covariance calls take
        self.n, self.m = int(x.shape[0]), int(z.shape[0])
        self.kernel, self.device_noise, self.jitter = kernel, bool(device_noise), float(jitter)
        self.approximation, self.mode = 'fitc' if key == 'fitc' else 'vfe', APPROXIMATIONS[key]
        self.lu = self.ws_u = self.info_u = self.lb = self.ws_b = self.info_b = self.gamma = None
        self._terms = None               # (lambda sums, the device scalars of the LML by name, q)
        self.bias = self.noise = self.sums = None        # a layer's block (fit_layer): device (q,), (1,) and float64 (3,)

    def _enqueue_fit(self, r, noise_dev=None):
        """The fit's device calls up to B = I + A^T W A (unfactored, in ``self.lb``), nothing read back: (A, w, lambda sums,
        c = A^T W r).  A (n x m) is the caller's to free.  ``noise_dev``: the noise variance as a device scalar, in place
        of ``kernel.noise``."""
        k, n, m = self.kernel, self.n, self.m
        self.lu = self.cov.gram(self._zs, self.jitter * k.sf)
        self.ws_u, self.info_u = dev.potrf(self.lu, m)
        a = self.cov.cross(self._xs, self._zs)
        dev.trsm_rows(self.lu, m, self.ws_u, a, n)
        _, w, sums = self.cov.lambda_pass(a, n, m, self._xs, self.mode, noise_dev)
        self.lb, c = dev.wsyrk_tn(a, n, m, w, r, diag_add=1.0)
        return a, w, sums, c

    def _enqueue_solve(self, c):
        """Factor L_B in place and gamma = L_B^-1 c; c is overwritten with b = B^-1 c = L_B^-T gamma."""
        self.ws_b, self.info_b = dev.potrf(self.lb, self.m)
        self.gamma = dev.potrs(self.lb, self.m, self.ws_b, c, want_z=True)

    def _enqueue_lml_terms(self, r, w, sums):
        """The device scalars of the LML, after :meth:`_enqueue_solve`."""
        scalars = dict(half_logdet_b=dev.logdet_half(self.lb, self.m), rwr=(r.double() ** 2 * w.double()[:, None]).sum(),
                       gg=(self.gamma.double() ** 2).sum())
        self._terms = (sums, scalars, int(r.shape[1]))

    def _raise_if_failed(self, info_u, bad, info_b):
        dev.raise_if_not_pd(info_u)
        if float(bad) > 0:
            raise np.linalg.LinAlgError("sparse GP: %d of the lambda_i = sf - q_i + noise are not positive" % int(bad))
        dev.raise_if_not_pd(info_b)

    def fit(self, r):
        """``r`` (n x q): residual targets on the device.  Nothing is read back but the two ``info`` words and the
        count of non-positive lambda."""
        r = r.contiguous()
        w, sums, c = self._enqueue_fit(r)[1:]            # A (n x m) is not needed after this: released here
        self._enqueue_solve(c)
        self._enqueue_lml_terms(r, w, sums)
        self._raise_if_failed(self.info_u, sums[2].item(), self.info_b)
        return self

    def fit_layer(self, y, f_bar, train_out, shared_bias=None, shared_noise=None, noise_fraction=NOISE_FRACTION,
                  noise_floor=NOISE_FLOOR):
        """The enqueue-only fit of a model layer's block: NOTHING is read back (``info_u``, ``info_b`` and ``sums[2]``,
        the count of non-positive lambda_i, stay on the device for :meth:`SparsePosterior.failure_flag`).  Targets, bias
        and noise are ``DenseBlock.fit``'s (``Posteriors.block_targets``).  While A is alive the block's training-point
        prediction A b + bias, b = L_B^-T gamma (what cimrgp_potrs leaves in c), is added into ``train_out`` (n x q) by
        cimrgp_sparse_tail_dev with A as W*; then A is released.  What stays -- L_u, L_B, their workspaces, gamma, bias,
        noise -- is m x m or smaller, whatever the model's ``keep_factors`` says."""
        self.bias, self.noise, r = block_targets(self.kernel, y, f_bar, shared_bias, shared_noise, noise_fraction, noise_floor)
        a, _, self.sums, c = self._enqueue_fit(r, self.noise)
        self._enqueue_solve(c)
        dev.sparse_tail_dev(None, a, self.n, self.m, c, self.kernel.sf, bias=self.bias, mean_out=train_out, accumulate=True)
        return self

    def hand_over_to(self, stream):
        """The block was fitted on a pool stream; its tensors are used on ``stream`` from now on."""
        for t in (self.z, self.lu, self.ws_u, self.info_u, self.lb, self.ws_b, self.info_b, self.gamma, self.bias, self.noise,
                  self.sums):
            if t is not None:
                t.record_stream(stream)

    def _lml_from(self, s0, s1, h, q):
        """The LML from host numbers: the first two lambda sums and ``h``, the scalars of :meth:`_enqueue_lml_terms` by name."""
        lml = (-0.5 * self.n * q * np.log(2 * np.pi) - 0.5 * q * s0 - q * float(h['half_logdet_b'])
               - 0.5 * float(h['rwr']) + 0.5 * float(h['gg']))
        if self.mode == 1:
            lml -= 0.5 * q * s1 / self.kernel.noise
        return float(lml)

    def log_marginal_likelihood(self):
        if self._terms is None:
            raise RuntimeError('call fit() before log_marginal_likelihood()')
        sums, scalars, q = self._terms
        s = sums.cpu().numpy()
        return self._lml_from(s[0], s[1], {name: t.item() for name, t in scalars.items()}, q)

    def _enqueue_g_fu(self, a, w, r, b):
        """The n x m chain in ONE buffer beside A: V = A L_B^-T, Y = V L_B^-1, G_A and G_fu = G_A L_u^-1 in place of one
        another.  Returns (G_fu, t, [sum h, sum t])."""
        n, m = self.n, self.m
        y = torch.empty_like(a)
        y.copy_(a)
        dev.trsm_rows(self.lb, m, self.ws_b, y, n)
        beta, t, gsums = dev.sparse_grad_rows(y, n, m, self.gamma, r, w, self.mode, self.kernel.noise)
        dev.trsm_rows_lt(self.lb, m, self.ws_b, y, n)
        dev.sparse_grad_combine(a, y, n, m, beta, b, w, t)
        dev.trsm_rows_lt(self.lu, m, self.ws_u, y, n)
        return y, t, gsums

    def _enqueue_g_uu(self, a, t, b, blow, q):
        """The m x m side: B^-1 from the identity, M = b b^T - q (I - B^-1) - 2 A^T diag(t) A and G_uu = -1/2 L_u^-T M L_u^-1
        (padded buffer).  A^T diag(t) A is cimrgp_wsyrk_tn with the signed weights t (FITC) or -(q / 2) (B - I) from
        ``blow``, B's lower triangle copied before it was factored (VFE; None under FITC).  Returns (M, G_uu)."""
        n, m, dt, device = self.n, self.m, self.z.dtype, self.z.device
        eye = torch.eye(m, dtype=dt, device=device)
        binv = dev.alloc_matrix(m, m, dt, device)
        binv.zero_()
        binv[:m, :m].fill_diagonal_(1.0)
        dev.trsm_rows(self.lb, m, self.ws_b, binv, m)
        dev.trsm_rows_lt(self.lb, m, self.ws_b, binv, m)
        low = torch.tril(dev.wsyrk_tn(a, n, m, t)[0][:m, :m]) if blow is None else blow
        full = low + torch.tril(low, -1).t()
        ata = full if blow is None else (-0.5 * q) * (full - eye)
        mm = b @ b.t() - q * (eye - binv[:m, :m]) - 2.0 * ata
        guu = dev.alloc_matrix(m, m, dt, device)
        guu[:m, :m] = 0.5 * (mm + mm.t())
        dev.trsm_rows_lt(self.lu, m, self.ws_u, guu, m)
        guu[:m, :m] = guu[:m, :m].t().clone()
        dev.trsm_rows_lt(self.lu, m, self.ws_u, guu, m)
        guu[:m, :m] = -0.25 * (guu[:m, :m] + guu[:m, :m].t())
        return mm, guu

    def _enqueue_pair_sums(self, g_fu, g_uu, want_z):
        """sum G o K, sum G o dK/dlog l and dZ of the scaled Z: K_fu's pairs, then K_uu's added (G_uu symmetric: scale 2 =
        -2 x -1).  Returns :meth:`BlockCovariance.pair_grad`'s (sums, lsums, dz)."""
        pairs = self.cov.pair_grad
        return pairs(self._zs, self._zs, g_uu, want_z, scale=2.0, into=pairs(self._xs, self._zs, g_fu, want_z))

    def _gradient_from(self, h, q):
        """``(lml, dtheta, grad_check)`` from the host values ``h`` of :meth:`lml_grad`'s read-back: host arithmetic only."""
        k, u = self.kernel, self.cov.u
        (s0, s1, _), (sum_h, sum_t) = h['sums'], h['gsums']
        gk, gl = h['psums'][0], h['psums'][1:]               # gl: one entry, or one per length-scale
        lml = self._lml_from(s0, s1, h, q)
        dnoise = k.noise * (sum_h + (0.5 * q / k.noise ** 2 * s1 if self.mode == 1 else 0.0))
        jit = self.jitter * k.sf * h['tr_guu']
        if u is None:
            # k is proportional to sf: the closed form, which the pairwise form must equal (checked by the GPU tests)
            dsf = 0.5 * h['tr_m'] + k.sf * sum_t
            check = dict(closed=float(dsf), pairwise=float(gk + jit + k.sf * sum_t))
            return lml, np.concatenate([[dsf], gl, [dnoise]]), check
        # 1/2 tr M = sum G o K over both matrices, whatever K is: the covariance's, the jitter's and the linear term's shares
        check = dict(closed=float(0.5 * h['tr_m']), pairwise=float(gk + jit + (u * h['lsums']).sum()))
        return lml, np.concatenate([[gk + jit + k.sf * sum_t], gl, [dnoise], u * (h['lsums'] + h['tx2'])]), check

    def lml_grad(self, r, want_z=True):
        """Fit on ``r`` (n x q, device) and return ``(lml, dtheta, dZ)``: the objective :meth:`log_marginal_likelihood`
        returns (bit for bit), its gradient w.r.t. (log sf, log l, log noise) as a NumPy (3,) array and, with ``want_z``,
        w.r.t. the inducing inputs as a device tensor (m x d), else None ("Gradients of the sparse
        objective").  With ``lengthscales`` the gradient is w.r.t. (log sf, log l_1 .. log l_d, log noise), a (d + 2,) array,
        and dZ is w.r.t. ``z`` in the caller's units.  With ``linear`` the gradient has d more entries at its end, w.r.t.
        log v_1 .. log v_d (dZ carries the linear part), and d / dlog sf is taken in its pairwise form: the closed form
        1/2 tr M + sf sum t holds only while k is proportional to sf.  ``grad_check`` keeps both forms of 1/2 tr M.
        The failure rules are :meth:`fit`'s.  A stays alive for the length of the call beside ONE more n x m buffer; one
        host read-back at the end (the info words, the lambda count and the scalars).  g of Matern 1/2 is taken as 0 at
        r = 0 (an inducing input on a training input or on another inducing input, where the objective has a kink): such
        pairs contribute nothing to dZ."""
        q, m = int(r.shape[1]), self.m
        r = r.contiguous()
        a, w, sums, b = self._enqueue_fit(r)
        blow = torch.tril(self.lb[:m, :m]) if self.mode == 1 else None   # VFE: B's lower triangle, before it is factored
        self._enqueue_solve(b)                           # potrs leaves B^-1 c = L_B^-T gamma in place of c
        self._enqueue_lml_terms(r, w, sums)
        g_fu, t, gsums = self._enqueue_g_fu(a, w, r, b)
        mm, guu = self._enqueue_g_uu(a, t, b, blow, q)
        del a                                            # n x m: not needed by the pair contractions
        psums, lsums, dz = self._enqueue_pair_sums(g_fu, guu, want_z)
        dz = self.cov.chain_rule(dz=dz)
        h = read_back(dict(self._terms[1], info_u=self.info_u, info_b=self.info_b, tr_m=torch.diagonal(mm).double().sum(),
                           tr_guu=torch.diagonal(guu[:m, :m]).double().sum()),
                      dict(sums=sums, gsums=gsums, psums=psums, lsums=lsums, tx2=self.cov.diag_grad(t, self._xs)))
        self._raise_if_failed(h['info_u'], h['sums'][2], h['info_b'])
        lml, dtheta, self.grad_check = self._gradient_from(h, q)
        return lml, dtheta, dz

    def chunk_rows(self, budget_bytes=None):
        """Test rows per pass of ``predict``: A* and W* within ``budget_bytes``."""
        return rows_within(self.z, budget_bytes)

    def predict(self, xs, mean=None, var=None, include_noise=False, budget_bytes=None):
        """Predictive mean into ``mean`` (ns x q) and variance into ``var`` (ns,) at ``xs`` (ns x d, device); either may
        be None.  Works in chunks of ``chunk_rows(budget_bytes)`` test rows: a row's result does not depend on the
        chunking."""
        if self.gamma is None:
            raise RuntimeError('call fit() before predict()')
        k, m, extra = self.kernel, self.m, self.kernel.noise if include_noise else 0.0
        accumulate = self.cov.seed_tail(xs, mean, var)
        for s0, s1, astar, wstar in self._star_chunks(xs, budget_bytes):
            dev.sparse_tail(astar if var is not None else None, wstar, s1 - s0, m, self.gamma if mean is not None else None, k.sf,
                            extra, None if mean is None else mean[s0:s1], None if var is None else var[s0:s1], accumulate)
        return mean, var

    def _star_chunks(self, xs, budget_bytes=None, cross=None):
        """(s0, s1, A*, W*) of every chunk of ``chunk_rows(budget_bytes)`` test rows: :func:`star_rows`' A* and
        W* = A* L_B^-T, in its two work buffers."""
        for s0, s1, astar, wstar in star_rows(self.cov, self._zs, self.lu, self.ws_u, self.m, xs, self.chunk_rows(budget_bytes), cross):
            wstar[:s1 - s0].copy_(astar[:s1 - s0])
            dev.trsm_rows(self.lb, self.m, self.ws_b, wstar, s1 - s0)
            yield s0, s1, astar, wstar

    def _ready_for(self, what):
        """The posterior queries below are the plugins': a model layer's block (``device_noise=True``) is refused, and so is
        a block with a linear term, before any device work."""
        if self.device_noise:
            raise TypeError('%s() of a sparse layer of the model (device_noise=True) is not yet supported' % what)
        if self.cov.lin is not None:
            raise TypeError('%s() of a sparse block with a linear term is not yet supported' % what)
        if self.gamma is None:
            raise RuntimeError('call fit() before %s()' % what)

    def grad_chunk_rows(self, budget_bytes=None):
        """Test rows per pass of ``predict_grad``: the d + 1 slabs of A* and of W* within ``budget_bytes``, a multiple of 256."""
        return rows_within(self.z, budget_bytes, int(self.z.shape[1]) + 1)

    def predict_grad(self, xs, mean_grad=None, var_grad=None, budget_bytes=None):
        """Gradients of :meth:`predict`'s mean and variance w.r.t. the test inputs ("Posterior queries of the
        sparse GP"): ``mean_grad`` (ns, d, q) and ``var_grad`` (ns, d), either may be None, at ``xs`` (ns x d, device, the
        caller's units -- with ``lengthscales`` the chain rule through x / l is applied).  K(X*, Z) and its d derivative
        slabs go through the SAME two row solves as :meth:`predict`, stacked as one (d + 1) rows x m operand; chunks of
        ``grad_chunk_rows(budget_bytes)`` test rows, a row's result does not depend on the chunking."""
        self._ready_for('predict_grad')
        k, m = self.kernel, self.m
        ns, d = int(xs.shape[0]), int(xs.shape[1])
        step = self.grad_chunk_rows(budget_bytes)
        ld, cap = dev.padded_ld(m), min(step, max(ns, 1))
        abuf = torch.empty((d + 1) * cap * ld, dtype=xs.dtype, device=xs.device)
        wbuf = torch.empty_like(abuf)
        for s0 in range(0, ns, step):
            s1 = min(ns, s0 + step)
            rows = s1 - s0
            a = abuf[:(d + 1) * rows * ld].view(d + 1, rows, ld)         # the slabs lie back to back: one operand of
            w = wbuf[:(d + 1) * rows * ld].view(d + 1, rows, ld)         # (d + 1) rows x m for the row solves
            dev.cov_cross_grad(self.cov.inputs(xs[s0:s1]).contiguous(), self._zs, k.l, k.sf, a, cov=k.cov)
            dev.trsm_rows(self.lu, m, self.ws_u, a.view(-1, ld), (d + 1) * rows)
            w.copy_(a)
            dev.trsm_rows(self.lb, m, self.ws_b, w.view(-1, ld), (d + 1) * rows)
            dev.sparse_tail_grad(a if var_grad is not None else None, w, rows, m, self.gamma if mean_grad is not None else None,
                                 None if mean_grad is None else mean_grad[s0:s1], None if var_grad is None else var_grad[s0:s1])
        self.cov.chain_rule(mean_grad=mean_grad, var_grad=var_grad)
        return mean_grad, var_grad

    def loo(self, r, mean=None, var=None, budget_bytes=None):
        """Leave-one-out prediction of the fit's own targets ``r`` (n x q, device): ``mean`` (n x q) and ``var`` (n,),
        either may be None.  Exact for FITC's covariance A A^T + Lambda (for VFE / DTC the same formula with Lambda =
        noise I): loo_mean_i = r_i - (r_i - mu_i) / (1 - h_i), loo_var_i = lambda_i / (1 - h_i), the variance of an
        observation, with the leverage h_i = w_i |V_i|^2.  A and V = A L_B^-T are recomputed in the chunks of
        :meth:`predict` over the training inputs; a row's result does not depend on the chunking.  One host read at the
        end: a row with 1 - h_i <= 0 raises LinAlgError."""
        self._ready_for('loo')
        k, r = self.kernel, r.contiguous()
        bad = torch.zeros(1, dtype=torch.int32, device=r.device)
        for s0, s1, a, v in self._star_chunks(self.x, budget_bytes):
            dev.sparse_loo(a, v, s1 - s0, self.m, self.gamma, r[s0:s1], k.sf, k.noise, self.mode, bad,
                           None if mean is None else mean[s0:s1], None if var is None else var[s0:s1])
        count = int(bad.item())
        if count > 0:
            raise np.linalg.LinAlgError("sparse GP leave-one-out: 1 - h_i is not positive for %d of the rows" % count)
        return mean, var

    def joint(self, xs, cov_out=None, samples=None, seed=0, include_noise=False, jitter=1e-6):
        """The joint predictive distribution at ``xs`` (ns x d, device): Sigma = K(X*, X*) - A* A*^T + W* W*^T, whose
        diagonal is :meth:`predict`'s variance.  ``cov_out`` (ns x ns): Sigma (+ noise I with ``include_noise``) is added
        to its lower triangle.  ``samples`` (cols x ns): chol(Sigma + jitter sf I) Z is added, Z_c = phi(seed, 0, c, .)
        (cimrgp_normal_fill), with the escalation rule of the exact blocks (``Posteriors.joint_blocks``, the same code).
        The ns x ns matrix and the rows A*, W* are held whole.  Returns the largest relative jitter used."""
        self._ready_for('joint')
        k, m, ns = self.kernel, self.m, int(xs.shape[0])
        if ns == 0:
            return 0.0
        xc = self.cov.inputs(xs).contiguous()
        astar = torch.empty((ns, dev.joint_ld(m, xs.dtype)), dtype=xs.dtype, device=xs.device)
        self.cov.cross(xc, self._zs, out=astar)
        dev.trsm_rows(self.lu, m, self.ws_u, astar, ns)
        wstar = astar.clone()
        dev.trsm_rows(self.lb, m, self.ws_b, wstar, ns)
        extra = k.noise if include_noise else 0.0

        def joint_cov(i, rel, carena, cws=None, info=None):
            dev.sparse_joint_cov(xc, k.l, k.sf, extra + (0.0 if rel is None else rel * k.sf), astar, wstar, m, carena[0],
                                 None if cws is None else cws[0], info, cov=k.cov)

        t_starts = torch.zeros(1, dtype=torch.int64, device=xs.device)
        return joint_blocks(joint_cov, [0], ns, t_starts, xs.dtype, xs.device, 0, cov_out, samples, seed, jitter)

    def predict_layer(self, xs, mean, var=None, add_noise=False, budget_bytes=None):
        """A model layer's block (:meth:`fit_layer`): ``mean`` (ns x q) += W* gamma + bias and, with ``var`` (ns,),
        var += sf - sum A*^2 + sum W*^2 (+ the block's noise, read on the device, with ``add_noise``), in the chunks of
        :meth:`predict`.  The mean alone takes the same route: weights L_u^-T b for the fused cross-covariance product
        would be of size ~ 1 / jitter and lose digits."""
        if self.gamma is None:
            raise RuntimeError('call fit_layer() before predict_layer()')
        for s0, s1, astar, wstar in self._star_chunks(xs, budget_bytes):
            dev.sparse_tail_dev(astar if var is not None else None, wstar, s1 - s0, self.m, self.gamma, self.kernel.sf,
                                bias=self.bias, extra_var_dev=self.noise if (add_noise and var is not None) else None,
                                mean_out=mean[s0:s1], var_out=None if var is None else var[s0:s1], accumulate=True)


def equivalent_exact_rows(n, m):
    """The size of the exact block that costs the flops of a sparse block, n_eq^3 / 3 = n m^2: what the stream pool's rule
    (``Posteriors.block_streams``, written for exact blocks) is asked with."""
    return int(round((3.0 * n * m * m) ** (1.0 / 3.0)))


class SparsePosterior(object):
    """One resolution of ``MultiResolutionGaussianProcess`` whose blocks are inducing-point GPs (:class:`SparseBlock`), the
    sparse twin of ``Posteriors.DensePosterior`` with the members the model uses ("Sparse layers in the
    multiresolution model").  ``kernel``: a ``KernelClass.SparseKernel``; ``layer``: the layer's number (it enters the
    draw of ``inducing='random'``); ``n_rows[l]``: rows of region l.  The blocks of a layer run on the stream pool; there is
    no batched C call for equal-sized sparse blocks."""

    def __init__(self, n_regions, dy, kernel, layer, n_rows, noise_region_specific=True, bias_region_specific=True):
        self.n_regions = int(n_regions)
        self.dy = int(dy)
        self.kernel = kernel
        self.layer = int(layer)
        self.n_rows = [int(n) for n in n_rows]
        self.noise_region_specific = noise_region_specific
        self.bias_region_specific = bias_region_specific
        self.blocks = [None] * self.n_regions
        self._z = {}                     # region -> (key of its inputs, Z on the device)
        self._scale = {}                 # region -> 1 / l on the device, of the last fit under an ARD base kernel
        self._greedy = {}                # inducing='greedy': region -> (key of its inputs, rows on the device, Z)
        self._greedy_kernel = kernel.kernel      # ... under the base kernel of the layer as constructed

    def needs_whole_layer(self):
        """As ``DensePosterior.needs_whole_layer``: a shared bias, or a shared noise taken from the targets."""
        return not (self.bias_region_specific and (self.noise_region_specific or self.kernel.noise is not None))

    def inducing_rows(self, region):
        """Row numbers, within region ``region``, of its inducing inputs: a function of the kernel's (inducing, seed), the
        layer, the region and its number of rows alone -- never of the rank count or of ownership.  ``inducing='greedy'``:
        the rows selected at the region's first fit, read back from the device here (a function of the region's inputs
        and the constructor's kernel alone); RuntimeError before that."""
        if self.kernel.inducing == 'greedy':
            if region not in self._greedy:
                raise RuntimeError('region %d of layer %d has no greedy rows yet: they are selected at its first fit'
                                   % (region, self.layer))
            return self._greedy[region][1].cpu().numpy()
        return self.kernel.inducing_rows(self.layer, region, self.n_rows[region])

    def _greedy_inputs(self, l, x_l):
        """Z of region l under ``inducing='greedy'``: the rows ``Inducing.greedy_rows`` picks among its inputs ``x_l`` under
        the kernel the layer was CONSTRUCTED with (an ARD base: on x / l at l = 1, as :meth:`_block` runs), selected once
        and kept on the device -- nothing is read back, the rows feed ``index_select``.  Trial and learned hyper-parameters
        leave them where they are (``self.kernel`` changes, ``self._greedy_kernel`` does not): the objective stays a smooth
        function of the hyper-parameters."""
        key = (x_l.data_ptr(), tuple(x_l.shape), x_l.dtype)
        if l not in self._greedy or self._greedy[l][0] != key:
            from .Inducing import greedy_rows
            if int(x_l.shape[0]) != self.n_rows[l]:
                raise ValueError('region %d of layer %d has %d rows, not %d' % (l, self.layer, x_l.shape[0], self.n_rows[l]))
            rows = greedy_rows(x_l.double(), self.kernel.num_inducing, self._greedy_kernel).rows
            self._greedy[l] = (key, rows, x_l.index_select(0, rows).contiguous())
        return self._greedy[l][2]

    def _inducing_inputs(self, l, x_l):
        """Z of region l: the rows :meth:`inducing_rows` of its inputs ``x_l``, gathered once and kept (the inputs of a
        model do not change; the learned hyper-parameters leave Z where it is)."""
        if self.kernel.inducing == 'greedy':
            return self._greedy_inputs(l, x_l)
        rows = self.inducing_rows(l)
        key = (x_l.data_ptr(), tuple(x_l.shape), x_l.dtype, rows.tobytes())
        if l not in self._z or self._z[l][0] != key:
            if int(x_l.shape[0]) != self.n_rows[l]:
                raise ValueError('region %d of layer %d has %d rows, not %d' % (l, self.layer, x_l.shape[0], self.n_rows[l]))
            idx = torch.as_tensor(rows).to(x_l.device)
            self._z[l] = (key, x_l.index_select(0, idx).contiguous())
        return self._z[l][1]

    def _block(self, l, x_l, z, kernel=None):
        """The block of region l: the layer's own for a fit (``kernel`` None; noise on the device), or one under the trial
        kernel ``kernel`` for the objective.  An ARD kernel ("ARD length-scales for the model's layers") runs at
        l = 1.0 on x / l and Z / l, Z being rows of x picked by index as ever: the objective's block does the scaling itself
        (``lengthscales=``); the layer's block, which takes no ``lengthscales``, is built on inputs scaled here, and
        :meth:`predict_layer` scales the test inputs with the ``self._scale[l]`` kept for it."""
        k = self.kernel
        base = k.kernel if kernel is None else kernel
        if not base.ard:
            if kernel is None:
                self._scale.pop(l, None)
            return SparseBlock(x_l, z, base, k.approximation, k.jitter, device_noise=kernel is None)
        if int(x_l.shape[1]) != len(base.l):
            raise ValueError('%d length-scales for inputs of dimension %d' % (len(base.l), int(x_l.shape[1])))
        unit = base.with_values(1.0, base.sf, base.noise)
        if kernel is not None:
            return SparseBlock(x_l, z, unit, k.approximation, k.jitter, lengthscales=base.l)
        self._scale[l], xs = unit_lengthscale(x_l, base.l)
        return SparseBlock(xs, scaled(z, self._scale[l]), unit, k.approximation, k.jitter, device_noise=True)

    def _fan(self, device, items):
        """The stream pool for blocks of (n, m) in ``items``."""
        return _Fanout(device, len(items), max(equivalent_exact_rows(n, m) for n, m in items))

    def update_scale_given_axis(self, y_mean, x, f_bar, train_out, owned=None, keep_factors=True):
        """Fit the ``owned`` regions (default all) on ``y_mean - f_bar`` and add their training-point predictions into
        ``train_out`` (lists indexed by region of device views, as for ``DensePosterior``), each by
        :meth:`SparseBlock.fit_layer` on a stream of the pool: enqueue-only, nothing is read back.  ``keep_factors`` changes
        nothing here: what a sparse block keeps is m x m (L_u, L_B, their workspaces) or smaller; the n x m matrix A is
        released at the end of every block's fit."""
        regions = list(range(self.n_regions) if owned is None else owned)
        shared_bias = shared_noise = None
        if self.needs_whole_layer():
            stats = dev.block_stats(DensePosterior._whole_layer(y_mean), DensePosterior._whole_layer(f_bar))
            if not self.bias_region_specific:
                shared_bias = stats[:self.dy]
            if not self.noise_region_specific and self.kernel.noise is None:
                shared_noise = dev.noise_from_stats(stats, self.dy, NOISE_FRACTION, NOISE_FLOOR * self.kernel.sf)
        if not regions:
            return
        zs = {l: self._inducing_inputs(l, x[l]) for l in regions}        # on the caller's stream, before the fan-out
        fan = self._fan(y_mean[regions[0]].device, [(int(x[l].shape[0]), int(zs[l].shape[0])) for l in regions])
        for l in regions:
            with torch.cuda.stream(fan.stream()):
                blk = self._block(l, x[l], zs[l])
                blk.fit_layer(y_mean[l], f_bar[l], train_out[l], shared_bias, shared_noise, NOISE_FRACTION, NOISE_FLOOR)
                if fan.pool:
                    blk.hand_over_to(fan.main)
            self.blocks[l] = blk
        fan.join()

    def predict_layer(self, x_all, xs, test_bounds, owned, mean, var, add_noise):
        """Accumulate the layer's predictive mean and (``var`` not None) variance at the test points: test block l = rows
        test_bounds[l] of ``xs``, served by training block l (:meth:`SparseBlock.predict_layer`), the owned blocks with
        test rows in flight together on the stream pool."""
        rest = []
        for l in sorted(owned):
            a, b = (int(v) for v in test_bounds[l])
            if b > a:
                rest.append((l, a, b))
        if not rest:
            return
        fan = self._fan(xs.device, [(b - a, self.blocks[l].m) for l, a, b in rest])
        for l, a, b in rest:
            with torch.cuda.stream(fan.stream()):
                xq = xs[a:b] if l not in self._scale else scaled(xs[a:b], self._scale[l])
                self.blocks[l].predict_layer(xq, mean[a:b], None if var is None else var[a:b], add_noise)
        fan.join()

    def layer_objective(self, ell, sf2, noise, y_mean, x, f_bar, owned=None):
        """As ``DensePosterior.layer_objective``: (lml, grad w.r.t. (log sf2, log ell, log noise), failure) of the layer's
        residual targets under (ell, sf2, noise), the sum of :meth:`SparseBlock.lml_grad` (``want_z=False``) over the
        ``owned`` regions; Z follows the layer's rule and stays fixed.  failure: 0, else 1 (a factor not positive definite
        or a non-positive lambda_i) or the watchdog code; lml and grad are meaningless when it is not 0.  ``ell`` a (d,)
        vector is ARD: grad has d + 2 entries, (log sf2, log l_1 .. log l_d, log noise)."""
        regions = list(range(self.n_regions) if owned is None else owned)
        q = self.dy
        trial = self.kernel.kernel.with_values(ell, sf2, noise)
        shared_bias = None
        if not self.bias_region_specific:
            shared_bias = dev.block_stats(DensePosterior._whole_layer(y_mean), DensePosterior._whole_layer(f_bar))[:q]

        def block(l):
            bias = shared_bias if shared_bias is not None else dev.block_stats(y_mean[l], f_bar[l])[:q]
            blk = self._block(l, x[l], self._inducing_inputs(l, x[l]), kernel=trial)
            return blk.lml_grad(dev.residual(y_mean[l], f_bar[l], bias), want_z=False)[:2]

        return sum_block_objectives(regions, block, np.size(ell) + 2)

    def _status(self, l):
        """Device float64 (3,): info_u, the count of non-positive lambda_i, info_b of block l; None if it has none."""
        blk = self.blocks[l]
        if blk is None or blk.info_u is None or blk.info_b is None or blk.sums is None:
            return None
        return torch.cat([blk.info_u.reshape(1).double(), blk.sums[2:3], blk.info_b.reshape(1).double()])

    def failure_flag(self, regions, out):
        """out[0] = the largest of info_u, info_b and the count of non-positive lambda_i over ``regions``: 0 = every block
        is fine, non-zero = failed, and a watchdog code (the largest value an ``info`` takes) stays recognisable.  Written
        on the device without a host synchronisation."""
        status = [s for s in (self._status(l) for l in regions) if s is not None]
        if status:
            out.copy_(torch.cat(status).max().to(out.dtype).reshape(1))
        return out

    def check(self, regions=None):
        """Raise for the first failed block of ``regions``, saying which of the three it was: ``numpy.linalg.LinAlgError``
        for K_uu + jitter sf I or B not positive definite or a non-positive lambda_i, RuntimeError for a watchdog code."""
        for l in (range(self.n_regions) if regions is None else regions):
            s = self._status(l)
            if s is None:
                continue
            info_u, bad, info_b = s.cpu().numpy()
            where = 'sparse layer %d, region %d' % (self.layer, l)
            for code, what in ((info_u, 'K_uu + jitter sf I'), (info_b, 'B = I + A^T Lambda^-1 A')):
                if dev.is_watchdog(code):
                    raise RuntimeError('cimrgp_potrf: schedule watchdog (%s, factor of %s)' % (where, what))
            if info_u != 0:
                raise np.linalg.LinAlgError('%s: K_uu + jitter sf I is not positive definite (leading minor of order %d)'
                                            % (where, int(info_u)))
            if bad > 0:
                raise np.linalg.LinAlgError('%s: %d of the lambda_i = sf - q_i + noise are not positive' % (where, int(bad)))
            if info_b != 0:
                raise np.linalg.LinAlgError('%s: B = I + A^T Lambda^-1 A is not positive definite (leading minor of order %d)'
                                            % (where, int(info_b)))
