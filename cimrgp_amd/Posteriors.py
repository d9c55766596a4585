"""Per-layer exact-GP posterior over the regions of one resolution.

Dense twin of the reference's ``Posterior`` (Posteriors.py:9-211): constructed
per layer, holds per-region state in lists indexed by region, and is updated
IN PLACE from lists indexed by region (Posteriors.py:35,81,113).  Where the
reference's ``update_scale_given_axis`` forms a diagonal precision and the
projected targets y~ (Posteriors.py:35-78), this class builds the Gram
matrix of the region under the layer's covariance (RBF or a half-integer Matern,
the kernel object's ``cov``), factors it and solves for the weights -- D1, D2, D3 of
SURVEY.md 8a' -- through the hand-written HIP kernels.
"""
import os

import numpy as np
import torch

from . import device as dev
from .Hyper import scaled, sum_block_objectives, unit_lengthscale

NOISE_FRACTION = 0.01    # RegressionInput.py:62: labels.var() * 0.01
NOISE_FLOOR = 1e-8       # x sf: keeps a constant-target block positive definite

#: equal-sized blocks of a layer up to this size are factored as ONE batch (same launches, grid.y =
#: block); larger blocks fill the machine on their own and keep the look-ahead schedule
BATCH_MAX_N = int(os.environ.get("CIMRGP_BATCH_MAX_N", "16384"))

# ---- independent blocks of one layer run concurrently (the reference's independent-over-l loop,
# Posteriors.py:35-59): a small pool of streams per device; blocks are dealt round-robin.
_POOLS = {}
#: upper bound on the streams of the pool (dist.share_one_gpu sets 1: ranks sharing one GPU)
MAX_BLOCK_STREAMS = 8


def block_streams(device, n_blocks, n_max):
    """How many blocks of a layer are in flight at once, and on which streams.  Small blocks are
    latency-bound (one queue each, ~10 % of the machine) and overlap almost perfectly; large ones
    already fill the machine with their trailing updates.  ``CIMRGP_BLOCK_STREAMS`` overrides."""
    env = os.environ.get("CIMRGP_BLOCK_STREAMS")
    if env is not None:
        want = int(env)
    elif n_max <= 5120:
        want = 8
    elif n_max <= 12288:
        want = 3
    elif n_max <= 20480:
        want = 2
    else:
        want = 1
    want = max(1, min(want, n_blocks, MAX_BLOCK_STREAMS))
    if want == 1:
        return []
    key = (torch.device(device).index, )
    pool = _POOLS.setdefault(key, [])
    while len(pool) < want:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:want]


class _Fanout(object):
    """Deal work items to pool streams: every stream starts after what is queued on the caller's
    stream, the caller's stream continues after all of them (events only, no host wait)."""

    def __init__(self, device, n_items, n_max):
        self.main = torch.cuda.current_stream(device)
        self.pool = block_streams(device, n_items, n_max)
        self.i = 0
        if self.pool:
            start = self.main.record_event()
            for s in self.pool:
                s.wait_event(start)

    def stream(self):
        if not self.pool:
            return self.main
        s = self.pool[self.i % len(self.pool)]
        self.i += 1
        return s

    def join(self):
        for s in self.pool:
            self.main.wait_stream(s)


def block_targets(kernel, y, f_bar, shared_bias, shared_noise, noise_fraction=NOISE_FRACTION, noise_floor=NOISE_FLOOR):
    """``(bias, noise, r)`` of one block, exact or sparse, fitted on ``y - f_bar`` (both (n x q) device views): bias (q,) =
    the column means of ``y - f_bar`` or ``shared_bias``; noise (1,) = ``kernel.noise``, else ``shared_noise``, else
    max(noise_fraction var(y - f_bar - bias), noise_floor sf); r = y - f_bar - bias.  All on the device, nothing read back."""
    q = int(y.shape[1])
    stats = None
    if shared_bias is None or (shared_noise is None and kernel.noise is None):
        stats = dev.block_stats(y, f_bar)
    bias = stats[:q] if shared_bias is None else shared_bias
    if kernel.noise is not None:
        noise = torch.full((1,), kernel.noise, dtype=y.dtype, device=y.device)
    elif shared_noise is not None:
        noise = shared_noise
    else:
        noise = dev.noise_from_stats(stats, q, noise_fraction, noise_floor * kernel.sf)
    return bias, noise, dev.residual(y, f_bar, bias)


class DenseBlock(object):
    """Device-resident state of one (resolution, region) block."""

    def __init__(self, x, kernel):
        if getattr(kernel, 'ard', False):
            # one length-scale per dimension: the layer object scales the inputs (DensePosterior); a block runs at one l
            raise TypeError('a DenseBlock takes an isotropic kernel: under ARD pass x / l and kernel.with_values(1.0, sf, noise)')
        self.x = x                       # (n x d) device view, normalised inputs
        self.n = int(x.shape[0])
        self.kernel = kernel
        self.lbuf = None                 # padded (n x ld) buffer holding L in its lower triangle
        self.ws = None                   # inverted diagonal blocks (potrf workspace)
        self.info = None                 # device int32, LAPACK convention
        self.alpha = None                # (n x q)  (K + noise I)^-1 r
        self.z = None                    # (n x q)  L^-1 r
        self.bias = None                 # (q,) device
        self.noise = None                # (1,) device
        self.r = None
        self.batch = None                # _FittedBatch this block's factor lives in (or None)
        self.batch_index = -1

    def fit(self, y, f_bar, train_out, shared_bias=None, shared_noise=None, keep_factor=True):
        """Fit on targets ``y - f_bar`` (both (n x q) device views); adds this
        block's training-point prediction into ``train_out`` (n x q)."""
        q = y.shape[1]
        k = self.kernel
        self.bias, self.noise, self.r = block_targets(k, y, f_bar, shared_bias, shared_noise)
        self.lbuf = dev.rbf_gram(self.x, k.l, k.sf, 0.0, lower_only=True, cov=k.cov)
        dev.add_diag(self.lbuf, self.n, self.noise)
        # the targets ride through the factorisation as q extra rows: z = L^-1 r comes out of the
        # same panel sweep (no separate forward solve), then one backward solve gives alpha
        q_rows = dev.alloc_matrix(q, self.n, y.dtype, y.device)
        q_rows[:q, :self.n] = self.r.t()
        self.ws, self.info = dev.potrf_rows(self.lbuf, self.n, q_rows, q)
        self.z = q_rows[:q, :self.n].t().contiguous()
        self.alpha = dev.solve_lt(self.lbuf, self.n, self.ws, self.z.clone())
        # K_noiseless alpha = r - noise * alpha: no second pass over the Gram matrix
        dev.train_mean(self.r, self.alpha, self.bias, self.noise, train_out, accumulate=True)
        if not keep_factor:
            self.lbuf = None
            self.ws = None
            self.z = None
        self.r = None

    def hand_over_to(self, stream):
        """The block was fitted on a pool stream; its tensors are used on ``stream`` from now on."""
        for t in (self.lbuf, self.ws, self.info, self.alpha, self.z, self.bias, self.noise):
            if t is not None:
                t.record_stream(stream)

    def _w_chunks(self, xs, chunk, what):
        """(s0, s1, W) for every ``chunk`` test points of ``xs``: W = K(xs[s0:s1], x) L^-T, the cross-Gram solved
        row-wise against the factor.  ``what`` names the caller's result in the error for a factor that was not kept."""
        if self.lbuf is None:
            raise RuntimeError('%s needs the Cholesky factor: fit with keep_factors=True' % what)
        k = self.kernel
        ns = xs.shape[0]
        for s0 in range(0, ns, chunk):
            s1 = min(ns, s0 + chunk)
            w = dev.rbf_cross(xs[s0:s1], self.x, k.l, k.sf, cov=k.cov)
            dev.trsm_rows(self.lbuf, self.n, self.ws, w, s1 - s0)
            yield s0, s1, w

    def joint_call(self, region, a, b):
        """This block as a batch of one for :func:`joint_run` at the test rows [a, b): its own inputs with start 0, its
        factor buffer as the arena."""
        if self.lbuf is None:
            raise RuntimeError('the joint covariance needs the Cholesky factor: fit with keep_factors=True')
        starts = torch.zeros(1, dtype=torch.int64, device=self.x.device)
        t_starts = torch.full((1,), int(a), dtype=torch.int64, device=self.x.device)
        one = _FittedBatch([region], self.n, starts, self.lbuf.unsqueeze(0), self.ws.unsqueeze(0), self.z.unsqueeze(0),
                           self.bias.unsqueeze(0), self.noise.reshape(1))
        return _JointCall(one, self.x, t_starts, int(b) - int(a))

    def predict(self, xs, mean_out, var_out=None, extra_var=0.0, chunk=16384, add_noise=False):
        """Accumulate this block's predictive mean (and latent variance) at ``xs``
        into ``mean_out`` (ns x q) / ``var_out`` (ns,).  ``add_noise``: add the block's noise
        variance, read from the device (no host round trip)."""
        k = self.kernel
        if var_out is None:
            dev.predict_mean(self.x, self.alpha, xs, k.l, k.sf, self.bias, out=mean_out, accumulate=True, cov=k.cov)
            return
        for s0, s1, w in self._w_chunks(xs, chunk, 'predictive variance'):
            dev.predict_from_w(w, s1 - s0, self.n, self.z, k.sf, extra_var, self.bias,
                               mean_out[s0:s1], var_out[s0:s1], accumulate=True,
                               extra_var_dev=self.noise if add_noise else None)

    def predict_grad(self, xs, mean_grad_out, var_grad_out=None, chunk=16384):
        """Accumulate this block's predictive gradients at ``xs`` ("Predictive gradients"):
        ``mean_grad_out`` (ns, d, q) += d mean / d xs from alpha, ``var_grad_out`` (ns, d) += d var / d xs from the rows
        beta = K(xs, x) K^-1 (a forward and a backward row solve per chunk of test points).  Either may be None."""
        k = self.kernel
        if var_grad_out is None:
            if mean_grad_out is not None:
                dev.cov_predict_grad(self.x, self.alpha, xs, k.l, k.sf, mean_grad=mean_grad_out, accumulate=True, cov=k.cov)
            return
        for s0, s1, w in self._w_chunks(xs, chunk, 'the gradient of the predictive variance'):
            dev.trsm_rows_lt(self.lbuf, self.n, self.ws, w, s1 - s0)
            dev.cov_predict_grad(self.x, self.alpha, xs[s0:s1], k.l, k.sf, beta=w,
                                 mean_grad=None if mean_grad_out is None else mean_grad_out[s0:s1],
                                 var_grad=var_grad_out[s0:s1], accumulate=True, cov=k.cov)

    def loo(self, y, mean_out, var_out=None):
        """Leave-one-out prediction of this block's own targets ("Leave-one-out cross-validation"):
        ``mean_out`` (n x q) = y - alpha / d, ``var_out`` (n,) = 1 / d with d = diag(K^-1) from row strips of L^-T
        (cimrgp_kinv_diag; at most LOO_SCRATCH_BYTES of scratch, which the result does not depend on).  ``y`` (n x q):
        the block's rows of the observations.  Point i is withheld from THIS block only: the coarser layers' prediction,
        the block's bias and its noise are those of the fit.  Either output may be None."""
        if self.lbuf is None:
            raise RuntimeError('leave-one-out needs the Cholesky factor: fit with keep_factors=True')
        d = dev.kinv_diag(self.lbuf, self.n, self.ws, LOO_SCRATCH_BYTES)
        dev.loo(y, self.alpha, d, mean_out, var_out)

    def log_marginal_likelihood(self, r_dot_alpha):
        """-1/2 r^T alpha - sum log L_ii - n/2 log 2pi, per output column summed."""
        half_logdet = float(dev.logdet_half(self.lbuf, self.n).item())
        q = self.alpha.shape[1]
        return -0.5 * r_dot_alpha - q * half_logdet - 0.5 * q * self.n * np.log(2 * np.pi)


def _layer_array(views, group):
    """The 2-D array (from the start of its storage) that the region views ``views[l]``, l in group, are row
    ranges of; None if they are not slices of one row-major array."""
    v0 = views[group[0]]
    st = v0.untyped_storage().data_ptr()
    rows = 0
    for l in group:
        v = views[l]
        if v.untyped_storage().data_ptr() != st or v.stride() != v0.stride() or v.stride(1) != 1 \
                or v.stride(0) != v.shape[1] or v.storage_offset() % v.stride(0) != 0:
            return None
        rows = max(rows, v.storage_offset() // v.stride(0) + v.shape[0])
    return torch.as_strided(v0, (int(rows), int(v0.shape[1])), v0.stride(), 0)


def scale_layer_inputs(x, lengthscales):
    """``(scale, x_all, views)`` of a layer's inputs under per-dimension length-scales (ARD): ``scale`` = 1 / lengthscales
    (``Hyper.unit_lengthscale``), ``views[l]`` = x[l] * scale for the region views ``x``.  When these are row ranges of one
    array (:func:`_layer_array`) there is ONE scaled copy ``x_all`` of it (rows x d) and the views are the same row ranges
    of that copy, so that the batched calls still address a block by one row offset; else x_all is None."""
    ls = np.asarray(lengthscales, dtype=np.float64)
    if ls.shape != (int(x[0].shape[1]),):
        raise ValueError('%d length-scales for inputs of dimension %d' % (ls.size, int(x[0].shape[1])))
    whole = _layer_array(x, list(range(len(x))))
    if whole is None:
        scale = unit_lengthscale(x[0], ls)[0]
        return scale, None, [scaled(v, scale) for v in x]
    scale, x_all = unit_lengthscale(whole, ls)
    rows = [v.storage_offset() // v.stride(0) for v in x]
    return scale, x_all, [x_all[r:r + int(v.shape[0])] for r, v in zip(rows, x)]


def _same_rows(arrays, group):
    """Whether region l starts at the same row (counted from the start of the storage) in every one of ``arrays``
    (lists of region views), for every l of ``group``: a view of y at a non-zero storage offset, say, does not."""
    def row_of(v):
        return v.storage_offset() // max(1, v.stride(0))
    return all(row_of(a[l]) == row_of(arrays[0][l]) for a in arrays[1:] for l in group)


def _groups_by_size(x, regions, arrays):
    """[(n, regions of n rows, sliced)] over ``regions``.  sliced: a batched call may address these blocks by ONE row
    offset into the layer's arrays -- every one of ``arrays`` (lists of region views) is a row-major 2-D array of which
    the region views are slices, at the same rows in all of them."""
    by_size = {}
    for l in regions:
        by_size.setdefault(int(x[l].shape[0]), []).append(l)
    return [(n_l, group, all(_layer_array(v, group) is not None for v in arrays) and _same_rows(arrays, group))
            for n_l, group in by_size.items()]


def _row_starts(sub, device, *arrays):
    """Device int64 tensor of the first row of every region of ``sub`` in the layer's arrays, which must be the same in
    all of ``arrays`` (lists of region views)."""
    def row_of(views, l):
        return views[l].storage_offset() // views[l].stride(0)
    rows = [row_of(arrays[0], l) for l in sub]
    if any(row_of(v, l) != r for v in arrays[1:] for l, r in zip(sub, rows)):
        raise ValueError('the region views of a layer must be the same row ranges of x, y, f_bar and train_out')
    return torch.tensor(rows, dtype=torch.int64).to(device, non_blocking=True)


def _ws_bytes(n, dtype):
    """Bytes of one block's factorisation workspace in an arena: a multiple of 16, never 0."""
    return max((dev.potrf_workspace_bytes(n, dtype) + 15) // 16 * 16, 16)


def free_device_bytes(device):
    """Bytes a new allocation on ``device`` can get: what the device reports free plus what the caching allocator holds
    without using it.  Every memory-bounded sub-batch split takes its budget as a fraction of this."""
    return torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _arena_geometry(y0, n, n_blocks, per_block_bytes, fraction):
    """(device, dtype, ld, ws_bytes, per_call) of the arenas that hold ``n_blocks`` (n x n) factors beside targets like
    ``y0``: padded pitch, workspace bytes per block, and how many blocks one call may take so that
    per_block_bytes(ld, ws_bytes, esz) each fit into ``fraction`` of the free memory."""
    device, dtype = y0.device, y0.dtype
    ld, ws_bytes = dev.padded_ld(n), _ws_bytes(n, dtype)
    per_block = per_block_bytes(ld, ws_bytes, y0.element_size())
    per_call = int(max(1, min(n_blocks, fraction * free_device_bytes(device) // per_block)))
    return device, dtype, ld, ws_bytes, per_call


class _FittedBatch(object):
    """Equal-sized blocks fitted together: their factors share one arena, so that a prediction can
    address block i at ``base + i * stride`` (cimrgp_layer_predict)."""

    def __init__(self, regions, n, starts, karena, ws_arena, z, bias, noise):
        self.regions, self.n, self.starts = list(regions), int(n), starts
        self.karena, self.ws_arena, self.z, self.bias, self.noise = karena, ws_arena, z, bias, noise

    def part(self, i0, nb):
        """Blocks [i0, i0 + nb) of the batch: views, nothing is copied."""
        s = slice(i0, i0 + nb)
        return _FittedBatch(self.regions[s], self.n, self.starts[s], self.karena[s], self.ws_arena[s], self.z[s],
                            self.bias[s], self.noise[s])

    def alpha(self):
        """(batch, n, q) weights K^-1 r, recomputed from a copy of z = L^-1 r: a batch keeps z, not alpha."""
        return dev.solve_lt_batched(self.karena, self.n, self.karena.stride(1), self.ws_arena, self.z.clone())


def plan_batched_calls(regions, owned, test_bounds, per_block_bytes, budget):
    """Which blocks of one batch go through batched calls.  ``regions``: the batch's region ids in arena order; ``owned``:
    the regions to compute; ``test_bounds[l]`` = (a, b): region l serves the test rows [a, b), or None for an operation on
    the training rows; ``per_block_bytes(ns)``: work memory of one block at ns test points; ``budget``: bytes one call may
    take.  Owned blocks with equally many test points form a group; a group goes through batched calls if it has test
    points, at least 2 blocks, and its arena indices are one contiguous run, cut into sub-batches of
    max(1, budget // per_block_bytes(ns)) blocks.  Returns (calls, covered): calls = [(i0, nb, ns, [first test row of
    each block])] over the arena indices [i0, i0 + nb) (ns None and no rows without test bounds), covered = the regions
    they serve.  Pure: touches no device."""
    by_ns = {}
    for i, l in enumerate(regions):
        if l in owned:
            a, b = (None, None) if test_bounds is None else (int(v) for v in test_bounds[l])
            by_ns.setdefault(None if a is None else b - a, []).append((i, a))
    calls, covered = [], set()
    for ns, items in by_ns.items():
        idx = [i for i, _ in items]
        contiguous = idx == list(range(idx[0], idx[0] + len(idx)))
        if (ns is not None and ns <= 0) or len(items) < 2 or not contiguous:
            continue
        per_call = int(max(1, min(len(items), budget // max(1, per_block_bytes(ns)))))
        for c0 in range(0, len(items), per_call):
            part = items[c0:c0 + per_call]
            calls.append((part[0][0], len(part), ns, [a for _, a in part if a is not None]))
        covered.update(regions[i] for i in idx)
    return calls, covered


#: escalations of a block's relative jitter (x 10 each) before a joint factorisation is given up
JOINT_RETRIES = 4
#: a retry starts from max(jitter, this) x 10: a zero jitter escalates to 1e-6 (GPy's jitchol starting value), ... 1e-3
JOINT_JITTER_FLOOR = 1e-7
#: bytes of standard normals one joint sampling call may hold
JOINT_Z_BYTES = 256 << 20


#: bytes of L^-T row strips one leave-one-out call may hold (the strip height follows from it; the result does not)
LOO_SCRATCH_BYTES = 512 << 20


class _JointCall(object):
    """Blocks of one layer that go through one cimrgp_layer_joint_cov call: the training side (a :class:`_FittedBatch`
    slice and ``x``, the array its starts index) and the test side (t_starts, ns)."""

    def __init__(self, batch, x, t_starts, ns):
        self.batch, self.x, self.t_starts, self.ns = batch, x, t_starts, int(ns)

    def part(self, i):
        """Block i alone (batch = 1): for a factorisation retried with more jitter."""
        return _JointCall(self.batch.part(i, 1), self.x, self.t_starts[i:i + 1], self.ns)


def joint_run(call, kernel, xs, layer, add_noise, cov_out=None, samples=None, seed=0, jitter=1e-6):
    """One call's share of the joint distribution ("Joint predictive covariance and posterior samples").
    ``cov_out`` (N* x N*): the blocks' Sigma (+ noise) is added to its lower triangle, no jitter.  ``samples`` (cols x
    N*): each block is factored with (jitter sf2 + noise) on its diagonal -- a block whose factorisation fails is
    retried alone with 10x the jitter (from JOINT_JITTER_FLOOR when it is smaller), at most JOINT_RETRIES times, then LinAlgError names the layer and region --
    and chol(.) Z is added, Z_b[c][i] = phi(seed, layer 2^32 + region, c, i).  Returns the largest relative jitter
    used (0.0 without samples)."""
    regions = call.batch.regions
    nb, ns, n = len(regions), call.ns, call.batch.n
    if ns <= 0 or nb == 0:
        return 0.0
    sf2 = float(kernel.sf)
    extra = call.batch.noise.to(xs.dtype) if add_noise else torch.zeros(nb, dtype=xs.dtype, device=xs.device)

    def joint_cov(i, rel, *out):
        c, ex = (call, extra) if i is None else (call.part(i), extra[i:i + 1])
        dev.layer_joint_cov(c.x, c.batch.starts, n, xs, c.t_starts, ns, kernel.l, sf2, c.batch.karena, c.batch.ws_arena,
                            ex if rel is None else ex + rel * sf2, *out, cov=kernel.cov)

    return joint_blocks(joint_cov, regions, ns, call.t_starts, xs.dtype, xs.device, layer, cov_out, samples, seed, jitter)


def joint_blocks(joint_cov, regions, ns, t_starts, dtype, device, layer, cov_out=None, samples=None, seed=0, jitter=1e-6):
    """What :func:`joint_run` does with the covariance blocks, whoever builds them (the exact blocks of a layer, or a
    sparse block: ``Sparse.SparseBlock.joint``).  ``joint_cov(i, rel, carena[, cws, info])`` fills the blocks of the call
    (``i`` None; carena (nb, ns, ldc)) or block ``i`` alone (the arenas' slices [i:i + 1]) with rel sf2 (+ noise) on the
    diagonal (``rel`` None: nothing but the noise) and, given ``cws`` and ``info``, factors them.  Block b serves the test
    rows from ``t_starts[b]`` (device int64)."""
    nb = len(regions)
    ldc = dev.joint_ld(ns, dtype)
    carena = torch.empty((nb, ns, ldc), dtype=dtype, device=device)
    if samples is None:
        joint_cov(None, None, carena)
        for i, a in enumerate(t_starts.cpu().tolist()):
            cov_out[a:a + ns, a:a + ns] += torch.tril(carena[i, :, :ns])
        return 0.0
    cws = torch.empty((nb, _ws_bytes(ns, dtype)), dtype=torch.uint8, device=device)
    info = torch.zeros(nb, dtype=torch.int32, device=device)
    joint_cov(None, jitter, carena, cws, info)
    used = float(jitter)
    for i in np.flatnonzero(info.cpu().numpy() != 0):          # info read once per call
        i, rel = int(i), max(float(jitter), JOINT_JITTER_FLOOR)
        for _ in range(JOINT_RETRIES):
            rel *= 10.0
            joint_cov(i, rel, carena[i:i + 1], cws[i:i + 1], info[i:i + 1])
            code = int(info[i].item())
            if code == 0:
                break
        if code != 0:
            if dev.is_watchdog(code):
                raise RuntimeError('cimrgp_potrf: schedule watchdog (joint factor of layer %d, region %d)'
                                   % (layer, regions[i]))
            raise np.linalg.LinAlgError('joint predictive covariance of layer %d, region %d is not positive definite '
                                        'with a relative jitter of %g (leading minor of order %d)'
                                        % (layer, regions[i], rel, code))
        used = max(used, rel)
    keys = torch.tensor([(int(layer) << 32) + int(l) for l in regions], dtype=torch.int64).to(device)
    cols = int(samples.shape[0])
    ldz = dev.joint_ld(ns, dtype)
    chunk = int(max(1, min(cols, JOINT_Z_BYTES // (nb * ldz * carena.element_size()))))
    z = torch.empty((nb, chunk, ldz), dtype=dtype, device=device)
    for c0 in range(0, cols, chunk):
        cc = min(chunk, cols - c0)
        dev.normal_fill(seed, keys, c0, cc, ns, z)
        dev.layer_sample(carena, ns, z, cc, t_starts, samples[c0:c0 + cc])
    return used


class DensePosterior(object):
    """One resolution: a list of :class:`DenseBlock`, updated in place."""

    def __init__(self, n_regions, dy, kernel, noise_region_specific=True, bias_region_specific=True):
        self.n_regions = int(n_regions)
        self.dy = int(dy)
        self.kernel = kernel
        self.noise_region_specific = noise_region_specific
        self.bias_region_specific = bias_region_specific
        self.blocks = [None] * self.n_regions
        self.batches = []                # _FittedBatch records of the last sweep (equal-sized blocks fitted together)

    # An ARD kernel (``kernel.ard``): the layer computes on inputs divided by the length-scales, under the same covariance
    # at l = 1.0 ("ARD length-scales for the model's layers").  The scaled copy of the training inputs belongs
    # to the kernel: setting ``kernel`` drops it, the next call that takes the region views makes it, and every call until
    # the kernel changes shares it.
    @property
    def kernel(self):
        return self._kernel

    @kernel.setter
    def kernel(self, kernel):
        self._kernel = kernel
        self._unit = kernel.with_values(1.0, kernel.sf, kernel.noise) if getattr(kernel, 'ard', False) else kernel
        self._ard = None                 # (key of the region views, scale, scaled layer array, scaled region views)

    def _scaled_train(self, x):
        """``x`` (region views) as the device calls take them: as given, or the views of the ARD copy."""
        if not self._kernel.ard:
            return x
        key = (x[0].untyped_storage().data_ptr(), x[0].dtype, tuple((v.storage_offset(), int(v.shape[0])) for v in x))
        if self._ard is None or self._ard[0] != key:
            self._ard = (key,) + scale_layer_inputs(x, self._kernel.l)
        return self._ard[3]

    def _scaled_test(self, x_all, xs):
        """``(x_all, xs)`` of a prediction: as given, or the ARD copy of the fit and ``xs`` in its units."""
        if not self._kernel.ard:
            return x_all, xs
        if self._ard is None:
            raise RuntimeError('an ARD layer predicts after it was fitted')
        return self._ard[2], scaled(xs, self._ard[1])

    def needs_whole_layer(self):
        """Whether the layer's fit reads statistics over ALL its regions (a shared bias, or a shared noise taken from
        the targets): such a layer needs the whole latent function on every rank (MRGP._fit)."""
        return not (self.bias_region_specific and (self.noise_region_specific or self.kernel.noise is not None))

    def update_scale_given_axis(self, y_mean, x, f_bar, train_out, owned=None, keep_factors=True):
        """``y_mean``, ``x``, ``f_bar``, ``train_out``: lists indexed by region of device
        views (the reference passes lists indexed by region too, Posteriors.py:35).
        ``owned``: iterable of the region ids this process computes (default all)."""
        regions = range(self.n_regions) if owned is None else owned
        shared_bias = shared_noise = None
        if self.needs_whole_layer():
            # layer-wide statistics over the concatenation of all regions (regions are
            # contiguous slices of one array: region 0's base with the total length)
            y_all, f_all = self._whole_layer(y_mean), self._whole_layer(f_bar)
            stats = dev.block_stats(y_all, f_all)
            if not self.bias_region_specific:
                shared_bias = stats[:self.dy]
            if not self.noise_region_specific and self.kernel.noise is None:
                shared_noise = dev.noise_from_stats(stats, self.dy, NOISE_FRACTION, NOISE_FLOOR * self.kernel.sf)
        regions = list(regions)
        self.batches = []
        if not regions:
            return
        x, k = self._scaled_train(x), self._unit
        # equal-sized small blocks: one batch per size (a uniform index set has at most two sizes per
        # layer, the last region taking the remainder, IndexSetGenerator.py:51-65)
        single = []
        for n_l, group, sliced in _groups_by_size(x, regions, (y_mean, x, f_bar, train_out)):
            if len(group) >= 2 and n_l <= BATCH_MAX_N and sliced:
                self._fit_batched(group, y_mean, x, f_bar, train_out, shared_bias, shared_noise, keep_factors)
            else:
                single.extend(group)
        if not single:
            return
        fan = _Fanout(y_mean[single[0]].device, len(single), max(int(x[l].shape[0]) for l in single))
        for l in single:
            with torch.cuda.stream(fan.stream()):
                blk = DenseBlock(x[l], k)
                blk.fit(y_mean[l], f_bar[l], train_out[l], shared_bias, shared_noise, keep_factor=keep_factors)
                if fan.pool:
                    blk.hand_over_to(fan.main)
            self.blocks[l] = blk
        fan.join()

    def _fit_batched(self, group, y_mean, x, f_bar, train_out, shared_bias, shared_noise, keep_factors):
        """Fit ``group`` (regions of equal size) with ONE C call per sub-batch (cimrgp_layer_fit): statistics,
        residual rows, Gram matrices, the batched factorisation with the residual rows carried, the batched
        backward solve and the training-point prediction are each launched once for all the blocks.  The
        matrices live in one arena (batch x n x ld); a group whose arena would not fit the free memory is cut
        into sub-batches (and the arena of a sub-batch is dropped at once when the factors are not kept)."""
        k = self._unit                   # x: what _scaled_train gave
        n = int(x[group[0]].shape[0])
        q = self.dy
        device, dtype, ld, ws_bytes, per_call = _arena_geometry(
            y_mean[group[0]], n, len(group), lambda ld, ws, esz: n * ld * esz + ws + 6 * q * ld * esz,
            0.8 if keep_factors else 0.4)
        # the layer's arrays: every region view is a slice of them (regions are contiguous ranges,
        # Inputs.py:57-60), so a block is a row offset into them
        y_all, x_all = _layer_array(y_mean, group), _layer_array(x, group)
        f_all, t_all = _layer_array(f_bar, group), _layer_array(train_out, group)
        for c0 in range(0, len(group), per_call):
            sub = group[c0:c0 + per_call]
            nb = len(sub)
            karena = torch.empty((nb, n, ld), dtype=dtype, device=device)
            ws_arena = torch.empty((nb, ws_bytes), dtype=torch.uint8, device=device)
            info = torch.zeros(nb, dtype=torch.int32, device=device)
            bias = torch.empty((nb, q), dtype=dtype, device=device)
            noise = torch.empty(nb, dtype=dtype, device=device)
            z = torch.empty((nb, n, q), dtype=dtype, device=device)
            alpha = torch.empty((nb, n, q), dtype=dtype, device=device)
            starts = _row_starts(sub, device, y_mean, x, f_bar, train_out)
            dev.layer_fit(x_all, y_all, f_all, t_all, starts, n, k.l, k.sf, -1.0 if k.noise is None else float(k.noise),
                          NOISE_FRACTION, NOISE_FLOOR * k.sf, shared_bias, shared_noise, karena, ws_arena, info, bias, noise,
                          z, alpha, cov=k.cov)
            batch = _FittedBatch(sub, n, starts, karena, ws_arena, z, bias, noise) if keep_factors else None
            if batch is not None:
                self.batches.append(batch)
            for i, l in enumerate(sub):
                blk = DenseBlock(x[l], k)
                blk.info = info[i:i + 1]
                blk.alpha = alpha[i]
                blk.bias = bias[i]
                blk.noise = noise[i:i + 1]
                if keep_factors:
                    blk.lbuf, blk.ws, blk.z = karena[i], ws_arena[i], z[i]
                    blk.batch, blk.batch_index = batch, i
                self.blocks[l] = blk

    def layer_objective(self, ell, sf2, noise, y_mean, x, f_bar, owned=None):
        """Log marginal likelihood of the layer's residual targets ``y_mean - f_bar`` (lists indexed by region of device
        views, as for :meth:`update_scale_given_axis`) under the covariance of ``self.kernel``'s class with
        (ell, sf2, noise), summed over the ``owned`` regions, and its gradient w.r.t. (log sf2, log ell, log noise).
        Each block's bias is its column means, or the whole layer's when ``bias_region_specific`` is False.
        Returns (lml, grad (3,), failure): failure = the largest LAPACK ``info`` of the blocks (0: all PD); lml and
        grad are meaningless when it is not 0.  Equal-sized blocks whose views are slices of one layer array go
        through ONE C call per sub-batch (cimrgp_layer_lml_grad_cov, one host read-back of its results); the others
        (larger than BATCH_MAX_N, or not slices) through the single-block composition
        (RegressionInput.log_marginal_likelihood), summed with the failure codes of Hyper.sum_block_objectives.
        ``ell`` a (d,) vector is ARD, whatever ``self.kernel`` is: grad has d + 2 entries ordered as ``Hyper.pack_theta``
        (sf, l_1 .. l_d, noise); the inputs are scaled once per evaluation and the batched call is
        cimrgp_layer_lml_grad_ard_cov."""
        from .RegressionInput import log_marginal_likelihood
        regions = list(range(self.n_regions) if owned is None else owned)
        q = self.dy
        cov = self.kernel.cov
        ard = np.ndim(ell) > 0
        n_grad = int(x[0].shape[1]) + 2 if ard else 3
        xb = scale_layer_inputs(x, ell)[2] if ard else x         # what the batched call takes
        shared_bias = None
        if not self.bias_region_specific:
            shared_bias = dev.block_stats(self._whole_layer(y_mean), self._whole_layer(f_bar))[:q]

        def single(l):
            bias = shared_bias if shared_bias is not None else dev.block_stats(y_mean[l], f_bar[l])[:q]
            return log_marginal_likelihood(x[l], dev.residual(y_mean[l], f_bar[l], bias), ell, sf2, noise, cov)

        lml, grad, failure = 0.0, np.zeros(n_grad), 0.0
        for n_l, group, sliced in _groups_by_size(xb, regions, (y_mean, xb, f_bar)):
            if n_l <= BATCH_MAX_N and sliced:
                a, g, f = self._objective_batched(group, ell, sf2, noise, y_mean, xb, f_bar, shared_bias)
            else:
                a, g, f = sum_block_objectives(group, single, n_grad)
            lml, grad, failure = lml + a, grad + g, max(failure, f)
        return lml, grad, failure

    def _objective_batched(self, group, ell, sf2, noise, y_mean, x, f_bar, shared_bias):
        """:meth:`layer_objective` of ``group`` (regions of equal size): sub-batches sized by the free memory as in
        :meth:`_fit_batched` (the K^-1 arena and the carried identity rows on top of the factor).  ``ell`` a vector: ``x``
        holds the inputs divided by it, and the records have d + 3 entries."""
        n = int(x[group[0]].shape[0])
        q = self.dy
        ard = np.ndim(ell) > 0
        width = int(x[group[0]].shape[1]) + 3 if ard else 4
        scratch = (dev.layer_lml_ard_scratch_bytes if ard else dev.layer_lml_scratch_bytes)(n, q, 1, y_mean[group[0]].dtype)
        device, dtype, ld, ws_bytes, per_call = _arena_geometry(
            y_mean[group[0]], n, len(group), lambda ld, ws, esz: 2 * n * ld * esz + ws + scratch, 0.8)
        y_all, x_all, f_all = _layer_array(y_mean, group), _layer_array(x, group), _layer_array(f_bar, group)
        lml, grad, failure = 0.0, np.zeros(width - 1), 0.0
        for c0 in range(0, len(group), per_call):
            sub = group[c0:c0 + per_call]
            nb = len(sub)
            starts = _row_starts(sub, device, y_mean, x, f_bar)
            karena = torch.empty((nb, n, ld), dtype=dtype, device=device)
            kinv = torch.empty((nb, n, ld), dtype=dtype, device=device)
            ws_arena = torch.empty((nb, ws_bytes), dtype=torch.uint8, device=device)
            info = torch.zeros(nb, dtype=torch.int32, device=device)
            out = torch.empty((nb, width), dtype=torch.float64, device=device)
            if ard:
                dev.layer_lml_grad_ard(x_all, y_all, f_all, starts, n, sf2, noise, shared_bias, karena, kinv, ws_arena, info, out,
                                       cov=self.kernel.cov)
            else:
                dev.layer_lml_grad(x_all, y_all, f_all, starts, n, ell, sf2, noise, shared_bias, karena, kinv, ws_arena, info, out,
                                   cov=self.kernel.cov)
            del karena, kinv, ws_arena
            res = torch.cat([out.reshape(-1), info.to(torch.float64)]).cpu().numpy()     # one read-back per call
            vals, infos = res[:width * nb].reshape(nb, width), res[width * nb:]
            if np.any(infos != 0):
                failure = max(failure, float(infos.max()))
                continue
            lml += float(vals[:, 0].sum())
            grad += vals[:, 1:].sum(axis=0)
        return lml, grad, failure

    def _run_layer(self, owned, test_bounds, device, per_block_bytes, budget, batched, single, fan_out=True):
        """Run one operation over the ``owned`` blocks of the layer.  Per batch of blocks fitted together,
        :func:`plan_batched_calls` picks the sub-batches (``per_block_bytes(batch, ns)`` bytes of work memory per block
        against ``budget()`` bytes, asked once per batch) and each goes to ``batched(part, t_starts, ns)``: a
        :meth:`_FittedBatch.part`, the device tensor of its blocks' first test rows and their common number of test
        points (both None when ``test_bounds`` is None: an operation on the training rows).  The owned blocks left over go
        to ``single(l, a, b)`` in region order -- (a, b) = test_bounds[l]; blocks without test points are passed over --
        dealt to the stream pool (``fan_out``), else on the caller's stream.  ``batched`` None: all one by one."""
        own, done = set(owned), set()
        for bt in (self.batches if batched is not None else ()):
            calls, covered = plan_batched_calls(bt.regions, own, test_bounds, lambda ns: per_block_bytes(bt, ns), budget())
            for i0, nb, ns, rows in calls:
                t_starts = None if ns is None else torch.tensor(rows, dtype=torch.int64).to(device, non_blocking=True)
                batched(bt.part(i0, nb), t_starts, ns)
            done |= covered
        rest = []
        for l in sorted(own - done):
            a, b = (None, None) if test_bounds is None else (int(v) for v in test_bounds[l])
            if a is None or b > a:
                rest.append((l, a, b))
        if not rest:
            return
        fan = _Fanout(device, len(rest) if fan_out else 1, max(self.blocks[l].n for l, _, _ in rest))
        for item in rest:
            with torch.cuda.stream(fan.stream()):
                single(*item)
        fan.join()

    def predict_layer(self, x_all, xs, test_bounds, owned, mean, var, add_noise):
        """Accumulate the layer's predictive mean and variance at the test points: test block l =
        rows test_bounds[l] of ``xs``, served by training block l (MRGP.py:782-803).  Blocks that were fitted
        together and have equally many test points go through ONE batched call per sub-batch
        (cimrgp_layer_predict); the others one by one on the stream pool (:meth:`_run_layer`).  ``var`` None: the mean
        alone, every block through the fused :func:`device.predict_mean`, which never forms W."""
        k = self._unit
        x_all, xs = self._scaled_test(x_all, xs)

        def batched(bt, t_starts, ns):
            dev.layer_predict(x_all, bt.starts, bt.n, xs, t_starts, ns, k.l, k.sf, bt.karena, bt.ws_arena, bt.z, bt.bias,
                              bt.noise if add_noise else None, mean, var, cov=k.cov)

        def single(l, a, b):
            self.blocks[l].predict(xs[a:b], mean[a:b], None if var is None else var[a:b], add_noise=add_noise)

        self._run_layer(owned, test_bounds, xs.device, lambda bt, ns: ns * dev.padded_ld(bt.n) * xs.element_size(),
                        lambda: 0.5 * free_device_bytes(xs.device), batched if var is not None else None, single)

    def predict_grad_layer(self, x_all, xs, test_bounds, owned, mean_grad, var_grad):
        """Accumulate the layer's predictive gradients at the test points (test block l = rows test_bounds[l] of ``xs``,
        served by training block l) through :meth:`_run_layer`: ONE cimrgp_layer_predict_grad_cov call per sub-batch
        (with :meth:`_FittedBatch.alpha`), the others one by one on the stream pool.
        An ARD layer's calls differentiate w.r.t. the SCALED test inputs: it computes into zeroed buffers of its own and adds
        them times 1 / l_k along d (d f / d x_k = (d f / d (x_k / l_k)) / l_k) into the buffers the layers share."""
        k = self._unit
        ard_out = None
        if self._kernel.ard:
            ard_out = (mean_grad, var_grad)
            x_all, xs = self._scaled_test(x_all, xs)
            mean_grad = None if mean_grad is None else torch.zeros_like(mean_grad)
            var_grad = None if var_grad is None else torch.zeros_like(var_grad)

        def batched(bt, t_starts, ns):
            dev.layer_predict_grad(x_all, bt.starts, bt.n, xs, t_starts, ns, k.l, k.sf, bt.karena, bt.ws_arena, bt.alpha(),
                                   mean_grad, var_grad, cov=k.cov)

        def single(l, a, b):
            self.blocks[l].predict_grad(xs[a:b], mean_grad[a:b], None if var_grad is None else var_grad[a:b])

        self._run_layer(owned, test_bounds, xs.device,
                        lambda bt, ns: (ns * dev.padded_ld(bt.n) + 2 * bt.n * self.dy) * xs.element_size(),
                        lambda: 0.5 * free_device_bytes(xs.device), batched, single)
        if ard_out is not None:
            scale = self._ard[1]
            if mean_grad is not None:
                ard_out[0].add_(mean_grad * scale[None, :, None])
            if var_grad is not None:
                ard_out[1].add_(var_grad * scale[None, :])

    def loo_layer(self, y_all, y, owned, mean, var):
        """Leave-one-out prediction of the layer's own targets by its ``owned`` blocks (:meth:`DenseBlock.loo`), written
        into the rows of ``mean`` (N x q) and ``var`` (N,) that each block's region covers.  ``y_all``: the (N x q)
        observations, ``y``: its region views (lists indexed by region, as for :meth:`update_scale_given_axis`).  Through
        :meth:`_run_layer` on the training rows: ONE cimrgp_kinv_diag_batched call per sub-batch (scratch bounded by
        LOO_SCRATCH_BYTES, with :meth:`_FittedBatch.alpha`), the others one by one on the stream pool."""
        def batched(bt, t_starts, ns):
            alpha = bt.alpha()
            d = dev.kinv_diag_batched(bt.karena, bt.n, bt.ws_arena, LOO_SCRATCH_BYTES)
            dev.loo(y_all, alpha, d, mean, var, starts=bt.starts)

        def single(l, a, b):
            r0 = y[l].storage_offset() // y[l].stride(0)
            r1 = r0 + int(y[l].shape[0])
            self.blocks[l].loo(y[l], mean[r0:r1], None if var is None else var[r0:r1])

        self._run_layer(owned, None, y_all.device, lambda bt, ns: dev.kinv_diag_scratch_bytes(bt.n, 256, y_all.dtype),
                        lambda: LOO_SCRATCH_BYTES, batched, single)

    def joint_layer(self, layer, x_all, xs, test_bounds, owned, add_noise, cov_out=None, samples=None, seed=0, jitter=1e-6):
        """This layer's share of the joint predictive distribution at the test points (test block l = rows
        test_bounds[l] of ``xs``, served by training block l), through :func:`joint_run`: :meth:`_run_layer` collects
        ONE cimrgp_layer_joint_cov call per sub-batch and the other blocks as batches of one; they run afterwards, in
        that order (``joint_run`` reads ``info`` back per call).  Returns the largest relative jitter used."""
        calls = []
        x_all, xs = self._scaled_test(x_all, xs)

        def per_block(bt, ns):
            ldc, ldw = dev.joint_ld(ns, xs.dtype), dev.joint_ld(bt.n, xs.dtype)
            return ns * (ldc + ldw) * xs.element_size() + dev.potrf_workspace_bytes(ns, xs.dtype) + 16

        self._run_layer(owned, test_bounds, xs.device, per_block, lambda: 0.4 * free_device_bytes(xs.device),
                        lambda bt, t_starts, ns: calls.append(_JointCall(bt, x_all, t_starts, ns)),
                        lambda l, a, b: calls.append(self.blocks[l].joint_call(l, a, b)), fan_out=False)
        used = 0.0
        for call in calls:
            used = max(used, joint_run(call, self._unit, xs, layer, add_noise, cov_out, samples, seed, jitter))
        return used

    @staticmethod
    def _whole_layer(views):
        base = views[0]
        total = sum(int(v.shape[0]) for v in views)
        return torch.as_strided(base, (total, base.shape[1]), base.stride())

    def failure_flag(self, regions, out):
        """out[0] = largest LAPACK ``info`` over ``regions`` (0 = all factorisations fine), written
        on the device without a host synchronisation."""
        infos = [self.blocks[l].info for l in regions if self.blocks[l] is not None and self.blocks[l].info is not None]
        if infos:
            out.copy_(torch.stack([i.reshape(()) for i in infos]).max().to(out.dtype).reshape(1))
        return out

    def check(self, regions=None):
        """Raise ``numpy.linalg.LinAlgError`` if any factorisation met a non-positive pivot."""
        for l in (range(self.n_regions) if regions is None else regions):
            if self.blocks[l] is not None and self.blocks[l].info is not None:
                dev.raise_if_not_pd(self.blocks[l].info)
