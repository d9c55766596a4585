"""Model orchestrator of the dense path: coarse-to-fine residual chain over
exact RBF GP blocks, sum-over-resolutions prediction.

API mirror of the reference's ``MultiResolutionGaussianProcess`` (MRGP.py:15-34
constructor keywords, ``fit`` :367, ``get_predicted_mean`` :805,
``get_central_moment2`` :816, ``get_test_likelihood`` :825, properties
``get_posterior`` / ``get_stats`` :359-365).  What changes is the per-block
arithmetic: where the reference expands each block in a sine basis and runs
mean-field updates, this class gives each block an exact RBF GP whose Gram
build, Cholesky and solves are hand-written HIP kernels (Posteriors.DenseBlock).
The structure is the reference's:
  * inputs z-scored once, globally (MRGP.py:278-295);
  * block (j, l) = contiguous index range of the index set (IndexSetGenerator.py:51-65);
  * layer j is fitted on  observations - f_bar,  f_bar = sum of the coarser
    layers' predictions at the training points (Stats.py:126-157,
    LatentOutputs.py:11-18, Posteriors.py:68);
  * prediction = sum over layers of the concatenated per-region predictions,
    test block (j, l) served by training block (j, l) (MRGP.py:757-803);
    variance likewise (MRGP.py:902-905).
With fixed hyper-parameters one sweep is exact, so ``fit`` runs a single sweep
whatever ``n_iter`` is (further sweeps would reproduce it bit for bit).
"""
import weakref

import numpy as np
import torch

from . import device as dev
from . import dist
from .Hyper import minimize_lml, pack_theta, unpack_theta
from .Inputs import Inputs
from .KernelClass import RBFKernel, DenseMaternKernel, SparseKernel
from .Posteriors import DensePosterior, NOISE_FRACTION
from .Sparse import SparsePosterior


class DenseStats(object):
    """Per-layer read-only view of what the reference keeps in ``Stats``
    (Stats.py:7-64): latent function per region, bias and noise per region."""

    def __init__(self, model, layer):
        # a proxy, not a reference: model -> stats_obj -> model would be a cycle, and a cycle keeps
        # tens of GB of Cholesky factors alive until the garbage collector happens to run
        self._m = weakref.proxy(model)
        self._j = layer
        self.n_regions = model.n_regions[layer]
        self.dy = model.dy

    @property
    def latent_f_mean(self):
        fb = self._m._f_bar_layers[self._j]
        return [fb[int(a):int(b)].double().cpu().numpy() for a, b in self._m.index_set_obj.bounds[self._j]]

    @property
    def bias_mean(self):
        return [None if b is None else b.bias.double().cpu().numpy() for b in self._m.posterior_obj[self._j].blocks]

    @property
    def noise_mean(self):
        """E[tau]: noise PRECISION, the reference's convention (Stats.py:30-35)."""
        return [None if b is None else 1.0 / float(b.noise.item()) for b in self._m.posterior_obj[self._j].blocks]


class MultiResolutionGaussianProcess(object):
    def __new__(cls, *args, **kwargs):
        """A basis-function object selects the reference's own reduced-rank blocks
        (``ReducedRank.ReducedRankMRGP``); without one the blocks are
        exact RBF GPs (this class)."""
        if cls is MultiResolutionGaussianProcess:
            basis = kwargs.get('basis_function_obj', args[3] if len(args) > 3 else None)
            if basis is not None:
                if kwargs.get('optimize_hyperparameters', args[24] if len(args) > 24 else False):
                    raise TypeError('not yet supported')
                from .ReducedRank import ReducedRankMRGP
                return object.__new__(ReducedRankMRGP)
        return object.__new__(cls)

    def __init__(self, train_xy,
                 n_basis=None,
                 index_set_obj=None,
                 basis_function_obj=None,
                 spectral_density_obj=None,
                 basis_interval_obj=None,
                 interval_factor=1,
                 adaptive_inputs=False,
                 standard_normalized_inputs=True,
                 axis_resolution_specific=False,
                 ard_resolution_specific=False,
                 noise_region_specific=True,
                 bias_region_specific=True,
                 noninformative_initialization=True,
                 snr_ratio=None,
                 full_x=None,
                 input_model=None,
                 forced_independence=False,
                 verbose=False,
                 dtype='f64',
                 device=None,
                 process_group=None,
                 keep_factors=True,
                 optimize_hyperparameters=False,
                 max_iters=1000):
        """``optimize_hyperparameters=True``: before each layer is fitted, its (variance, length-scale, noise) are learned
        by L-BFGS-B on the sum over its regions of the log marginal likelihood of the layer's residual targets (see
        :meth:`_learn_layer`); at most ``max_iters`` iterations per layer.  Only for the dense blocks (no
        ``basis_function_obj``).

        A layer whose entry of ``spectral_density_obj`` is a ``SparseKernel`` is SPARSE: its blocks are inducing-point GPs
        (``Sparse.SparsePosterior``; DESIGN.md, "Sparse layers in the multiresolution model"), mixed freely with exact
        layers in the one residual chain.  FP64 only."""
        if optimize_hyperparameters and basis_function_obj is not None:
            raise TypeError('not yet supported')
        if int(max_iters) < 1:
            raise ValueError('max_iters must be at least 1')
        self.optimize_hyperparameters = bool(optimize_hyperparameters)
        self.max_iters = int(max_iters)
        self.optimizer_results = [None] * (index_set_obj.get_n_resolutions() + 1 if index_set_obj is not None else 0)
        self.verbose = verbose
        self.forced_independence = forced_independence
        if forced_independence is not True and (axis_resolution_specific or ard_resolution_specific):
            raise TypeError("not yet supported")
        if index_set_obj is None:
            raise ValueError('index_set_obj is required')
        self.adaptive_inputs = adaptive_inputs
        self.standard_normalized_inputs = standard_normalized_inputs
        self.noise_region_specific = noise_region_specific
        self.bias_region_specific = bias_region_specific
        self.keep_factors = keep_factors

        self.n_layers = index_set_obj.get_n_resolutions() + 1
        self.index_set_obj = index_set_obj
        self.n_basis = n_basis
        x_train = np.asarray(train_xy[0], dtype=np.float64)
        y_train = np.asarray(train_xy[1], dtype=np.float64)
        self.observations = y_train
        self.dy = y_train.shape[1]
        if self.dy < 2:
            raise ValueError('output dimension must be greater than 1')
        if x_train.shape[0] != index_set_obj.sample_length:
            raise ValueError('index set was built for a different number of samples')

        x_train, self.full_x, self.mean_x_train, self.std_x_train = self._normalize_inputs(x_train, full_x)

        if spectral_density_obj is None:
            spectral_density_obj = RBFKernel()
        if isinstance(spectral_density_obj, list):
            if len(spectral_density_obj) != self.n_layers:
                raise ValueError('spectral_density_obj must be a list of the same length as the number of '
                                 'resolutions + 1')
            self.spectral_density_obj = spectral_density_obj
        else:
            self.spectral_density_obj = [spectral_density_obj] * self.n_layers
        for k in self.spectral_density_obj:
            if not isinstance(k, (RBFKernel, DenseMaternKernel, SparseKernel)):
                # a spectral density without a basis-function object (MaternKernel: general nu, no closed form):
                # neither path applies
                raise TypeError('spectral_density_obj must be an RBFKernel or a DenseMaternKernel (nu = 1/2, 3/2, 5/2) '
                                'when basis_function_obj is None')
            if isinstance(k, SparseKernel) and dev.as_torch_dtype(dtype) != torch.float64:
                # cond(K_uu + eps sf I) ~ m / eps exceeds what FP32 holds at eps = 1e-6
                raise TypeError('not yet supported')
            if k.ard and len(k.l) != x_train.shape[1]:
                raise ValueError('an ARD kernel with %d length-scales for inputs of dimension %d'
                                 % (len(k.l), x_train.shape[1]))
        if snr_ratio is not None:
            # reference: initial noise variance of layer 0 from an SNR (MRGP.py:196-199,966-971)
            self.spectral_density_obj = list(self.spectral_density_obj)
            k0 = self.spectral_density_obj[0]
            self.spectral_density_obj[0] = k0.with_noise(self._compute_initial_noise_var_from_snr(y_train, snr_ratio))

        self.device = dev.require_gpu(device)
        self.dtype = dev.as_torch_dtype(dtype)
        self.group = process_group
        self.rank, self.world_size = dist.world(process_group)

        # learned input warp x -> regular grid (Inputs.py:8-55): an exact RBF GP fitted on the GPU
        self.input_obj = Inputs(x=x_train, index_set=index_set_obj, learn_inputs=self.adaptive_inputs,
                                full_x=self.full_x, input_model=input_model)
        self._x_dev = dev.to_device(self.input_obj.x, self.dtype, self.device)
        self.dx = self.input_obj.x.shape[1]
        self.n_regions = [len(layer) for layer in index_set_obj.bounds]
        self.n_samps = [[int(b - a) for a, b in layer] for layer in index_set_obj.bounds]
        self.x = [[self._x_dev[int(a):int(b)] for a, b in index_set_obj.bounds[j]] for j in range(self.n_layers)]
        self._y = dev.to_device(y_train, self.dtype, self.device)
        # nested ownership: layers >= self._first_local exchange nothing during the fit (dist.plan_layers)
        self.owner, self._first_local = dist.plan_layers(index_set_obj.bounds, self.world_size)

        self.posterior_obj = [self._new_posterior(j) for j in range(self.n_layers)]
        self.stats_obj = [DenseStats(self, j) for j in range(self.n_layers)]
        self._f_bar_layers = [None] * self.n_layers
        self._fitted = False
        self.last_joint_jitter = [0.0] * self.n_layers
        self.lower_bound = []
        self.lower_bound_layer = [[] for _ in range(self.n_layers)]

    # ------------------------------------------------------------------ helpers
    def _new_posterior(self, j):
        """The layer object of layer j: sparse if its kernel is a ``SparseKernel``, else dense."""
        k = self.spectral_density_obj[j]
        if isinstance(k, SparseKernel):
            return SparsePosterior(self.n_regions[j], self.dy, k, j, self.n_samps[j], self.noise_region_specific,
                                   self.bias_region_specific)
        return DensePosterior(self.n_regions[j], self.dy, k, self.noise_region_specific, self.bias_region_specific)

    def _is_sparse(self, j):
        return isinstance(self.posterior_obj[j], SparsePosterior)

    def _refuse_sparse(self, index_set):
        """TypeError if a layer that serves test points under ``index_set`` (None: layer 0 alone) is sparse: for results
        the sparse blocks do not give yet.  Host only, the same on every rank."""
        serving = 1 if index_set is None else min(self.n_layers, index_set.get_n_resolutions() + 1)
        if any(self._is_sparse(j) for j in range(serving)):
            raise TypeError('not yet supported')

    def _normalize_inputs(self, x_train, full_x):
        x = x_train if full_x is None else np.asarray(full_x, dtype=np.float64)
        if self.standard_normalized_inputs is True:
            std_x_train = np.std(x, 0)
            std_x_train[std_x_train == 0] = 1
            mean_x_train = np.mean(x, 0)
            x_train = (x_train - mean_x_train) / std_x_train
            if full_x is not None:
                full_x = (x - mean_x_train) / std_x_train
        else:
            mean_x_train = None
            std_x_train = None
        return x_train, full_x, mean_x_train, std_x_train

    def _slices(self, t, layer, bounds=None):
        bounds = self.index_set_obj.bounds if bounds is None else bounds
        return [t[int(a):int(b)] for a, b in bounds[layer]]

    def _owned(self, layer):
        return [l for l in range(self.n_regions[layer]) if self.owner[layer][l] == self.rank]

    @property
    def get_posterior(self):
        return self.posterior_obj

    @property
    def get_stats(self):
        return self.stats_obj

    # ---------------------------------------------------------------------- fit
    def fit(self, n_iter=1, tol=1e-3, min_iter=10):
        self._fit()

    # ------------------------------------------------- per-layer hyper-parameters
    def layer_log_marginal_likelihood(self, layer, ell, sf, noise):
        """(lml, grad) of layer ``layer`` at (ell, sf = variance, noise) on the residual targets of the last fit
        (y - f_bar of that layer, the layer's bias rule), summed over all regions and ranks; grad is w.r.t.
        (log sf, log ell, log noise).  ``ell`` a (d,) vector, whatever the layer's own kernel: one length-scale per input
        dimension (ARD), grad w.r.t. (log sf, log l_1 .. log l_d, log noise).  Collective: every rank calls it.  Raises
        LinAlgError if a block is not PD."""
        if not self._fitted:
            raise RuntimeError('call fit() before evaluating a layer objective')
        lml, grad, failure = self._layer_objective(layer, self._f_bar_layers[layer], ell, sf, noise)
        if failure != 0.0:
            raise np.linalg.LinAlgError('Matrix is not positive definite (a block of layer %d)' % layer)
        return lml, grad

    def _layer_objective(self, j, f_bar, ell, sf, noise):
        """Sum over this rank's blocks of layer j, then ONE all-reduce of [lml | grad | failure] over the ranks, so that
        every rank sees the same objective.  A watchdog code raises RuntimeError on every rank."""
        post = self.posterior_obj[j]
        lml, grad, failure = post.layer_objective(ell, sf, noise, self._slices(self._y, j), self.x[j], self._slices(f_bar, j),
                                                  self._owned(j))
        if self.world_size > 1:
            buf = torch.tensor([lml] + list(grad) + [failure], dtype=torch.float64, device=self.device)
            dist.allreduce_sum_(buf, self.group)
            vals = buf.cpu().numpy()
            lml, grad, failure = float(vals[0]), vals[1:-1], float(vals[-1])       # grad: 3 entries, or d + 2 under ARD
        if dev.is_watchdog(failure):
            raise RuntimeError('cimrgp_potrf: schedule watchdog while evaluating the objective of layer %d' % j)
        return lml, np.asarray(grad, dtype=np.float64), failure

    def _learn_layer(self, j, f_bar):
        """L-BFGS-B (SciPy) on -sum_l LML_l over theta = (log sf, log l, log noise) of layer j, from the constructor's
        kernel (noise: its own, else NOISE_FRACTION * sf); the layer is then fitted with a NEW kernel object of the
        same class holding the learned values (the noise fixed and shared by the layer's regions).  A trial point at
        which a block is not positive definite is a failed point of ``Hyper.minimize_lml``.  With several ranks every
        evaluation costs one small all-reduce.
        A sparse layer learns its base kernel's values (the inducing inputs stay where the layer's rule puts them) and
        the learned kernel is wrapped in a ``SparseKernel`` with the same settings.
        An ARD kernel learns its d length-scales: theta = (log sf, log l_1 .. log l_d, log noise), from the constructor's
        vector (``RBFKernel(l=[1., 1.])`` starts an ARD search from an isotropic point)."""
        k0 = self.spectral_density_obj[j]
        n_ell = len(k0.l) if k0.ard else None

        def objective(theta):
            lml, grad, failure = self._layer_objective(j, f_bar, *unpack_theta(theta, n_ell))
            return None if failure != 0.0 else (lml, grad)

        theta0 = pack_theta(k0.sf, k0.l, k0.noise if k0.noise is not None else NOISE_FRACTION * k0.sf)
        res = minimize_lml(objective, theta0, self.max_iters)
        self.optimizer_results[j] = res
        self.posterior_obj[j].kernel = k0.with_values(*unpack_theta(res.x, n_ell))

    def _fit(self):
        n, q = self._y.shape
        if self.optimize_hyperparameters:
            # a re-fit starts again from the constructor's kernels
            for j in range(self.n_layers):
                self.posterior_obj[j].kernel = self.spectral_density_obj[j]
            self.optimizer_results = [None] * self.n_layers
        f_bar = torch.zeros_like(self._y)
        self._layer_events = [torch.cuda.Event(enable_timing=True) for _ in range(self.n_layers + 1)]
        failed = torch.zeros(self.n_layers, dtype=self.dtype, device=self.device)
        # Layers from self._first_local on are LOCAL (dist.plan_layers): a rank's blocks lie inside row ranges whose
        # coarser predictions it computed itself, so the residual chain needs no exchange there; their predictions
        # (and failure flags) are assembled on every rank by ONE all-reduce after the sweep.
        # NOT when a layer takes statistics over ALL its regions (shared bias / shared noise: bias_region_specific or
        # noise_region_specific False): those read the whole latent function, which a rank holds on its own ranges
        # only while the layers are local -- then every layer is exchanged as it is fitted (round 5).
        local_from = self._first_local if self.world_size > 1 else self.n_layers
        if any(p.needs_whole_layer() for p in self.posterior_obj[local_from:]):
            local_from = self.n_layers
        self._local_from = local_from
        n_local = max(0, self.n_layers - local_from) if self.world_size > 1 else 0
        # every local layer writes a zero-offset (N x q) array of its own (the batched fit addresses a block by ONE row
        # offset from the start of the storage: a view into a shared buffer at an odd offset would disable it);
        # the flags sit in a small tensor; both are copied into ONE flat buffer for the single collective
        local_pred = [torch.zeros((n, q), dtype=self.dtype, device=self.device) for _ in range(n_local)]
        local_flag = torch.zeros(max(n_local, 1), dtype=self.dtype, device=self.device)
        for j in range(self.n_layers):
            self._layer_events[j].record()
            self._f_bar_layers[j] = f_bar
            is_local = j >= local_from and n_local > 0
            if is_local:
                layer_pred, flag = local_pred[j - local_from], local_flag[j - local_from:j - local_from + 1]
                buf = None
            else:
                # [layer's training-point prediction (N x q) | failure flag]: ONE buffer, one collective
                buf = torch.zeros(n * q + 1, dtype=self.dtype, device=self.device)
                layer_pred, flag = buf[:n * q].view(n, q), buf[n * q:]
            owned = self._owned(j)
            if self.optimize_hyperparameters:
                self._learn_layer(j, f_bar)
            self.posterior_obj[j].update_scale_given_axis(
                y_mean=self._slices(self._y, j), x=self.x[j], f_bar=self._slices(f_bar, j),
                train_out=self._slices(layer_pred, j), owned=owned, keep_factors=self.keep_factors)
            # A non-PD block must fail on EVERY rank, not only on its owner (whose exception
            # would leave the others blocked in the collective): the blocks' LAPACK-style info
            # words ride in the same all-reduce and every rank raises after it.
            self.posterior_obj[j].failure_flag(owned, out=flag)
            if not is_local:
                # residual chain (Stats.py:126-157): every rank needs the whole layer's prediction
                dist.allreduce_sum_(buf, self.group)
                failed[j:j + 1].copy_(buf[n * q:])           # read ONCE, after the sweep: the fit stays enqueue-only
            f_bar = f_bar + layer_pred                       # local layers: valid on this rank's own ranges, all it reads
        if n_local:
            tail = torch.cat([t.reshape(-1) for t in local_pred] + [local_flag[:n_local]])
            dist.allreduce_sum_(tail, self.group)
            # the latent function of every layer, now complete on every rank
            f_bar = self._f_bar_layers[local_from]
            for j in range(local_from, self.n_layers):
                k = j - local_from
                self._f_bar_layers[j] = f_bar
                f_bar = f_bar + tail[k * n * q:(k + 1) * n * q].view(n, q)
            failed[local_from:].copy_(tail[n_local * n * q:])
        self._layer_events[self.n_layers].record()
        # (a host read per layer made the device wait for the host's enqueue of the next layer: 2-3 ms on the
        # fine layers of config 4.  After a failed factorisation the later layers run on garbage -- harmless:
        # every kernel is bounded and flags its own `info` -- and the first failing layer is the one reported.)
        flags = failed.cpu().numpy()
        if np.any(flags != 0.0):
            j = int(np.flatnonzero(flags != 0.0)[0])
            self.posterior_obj[j].check(self._owned(j))      # the owner reports the leading minor
            if dev.is_watchdog(flags[j]):                    # a schedule failure on another rank: not "not PD"
                raise RuntimeError('cimrgp_potrf: schedule watchdog (a block of layer %d owned by another rank)' % j)
            raise np.linalg.LinAlgError('Matrix is not positive definite (a block of layer %d '
                                        'owned by another rank)' % j)
        self._f_bar_final = f_bar
        self._fitted = True

    def layer_fit_ms(self):
        """Device time of each layer of the last sweep (events on the fit's stream)."""
        torch.cuda.synchronize(self.device)
        ev = self._layer_events
        return [float(ev[j].elapsed_time(ev[j + 1])) for j in range(self.n_layers)]

    # ------------------------------------------------------------------ predict
    def _prepare_test(self, test_x):
        test_x = np.asarray(test_x, dtype=np.float64)
        if self.standard_normalized_inputs is True:
            test_x = (test_x - self.mean_x_train) / self.std_x_train
        if self.adaptive_inputs is True:                 # MRGP.py:770-778
            test_x = self.input_obj.warp(test_x, self.full_x)
        return dev.to_device(test_x, self.dtype, self.device)

    def _check_index_set(self, index_set, number_of_regions):
        if index_set.get_n_resolutions() > self.index_set_obj.get_n_resolutions():
            raise ValueError('resolution in the test index set must be smaller or equal to that in the '
                             'train set.')
        if number_of_regions is None:
            if getattr(self.index_set_obj, 'divider', None) != getattr(index_set, 'divider', None):
                raise ValueError('divider on the training index_set must be'
                                 ' the same as in the test index_set.')
        else:
            if (self.n_regions == number_of_regions) is False:
                raise ValueError('number of regions in the training must be the same as test.')
        for j in range(index_set.get_n_resolutions() + 1):
            if len(index_set.bounds[j]) != self.n_regions[j]:
                raise ValueError('number of regions in the training must be the same as test.')

    def _test_points(self, test_x, index_set=None, number_of_regions=None):
        """What a prediction starts with: the test index set (if given) is checked against the training one, the model
        must be fitted, and the test inputs go through the training inputs' transformations onto the device."""
        if index_set is not None:
            self._check_index_set(index_set, number_of_regions)
        if not self._fitted:
            raise RuntimeError('call fit() before predicting')
        return self._prepare_test(test_x)

    def _test_layers(self, index_set, ns, include_noise=True):
        """[(layer, test bounds, add noise, owned regions)] of the layers that serve ``ns`` test points and have blocks
        of this rank: every layer of ``index_set``, the finest adding its blocks' noise.  Without an index set every
        prediction is taken from resolution 0 (MRGP.py:726-755), which presumes ONE root region -- it serves all the test
        points and no noise is added; with a multi-region first layer the test points need an index set."""
        if index_set is None:
            if self.n_regions[0] != 1:
                raise ValueError('index_set_obj is required when the first layer has more than one region')
            layers = [(0, [(0, ns)], False)]
        else:
            n_layers = index_set.get_n_resolutions() + 1
            layers = [(j, index_set.bounds[j], include_noise and j == n_layers - 1) for j in range(n_layers)]
        return [(j, bounds, add_noise, self._owned(j)) for j, bounds, add_noise in layers if self._owned(j)]

    def _sum_shares(self, fused, share):
        """Run ``share()``, which adds this rank's blocks into the zero-initialised ``fused`` = [payload | not positive
        definite | any other failure], then sum ``fused`` over the ranks in ONE collective.  An exception of ``share``
        (LinAlgError, the factorisation's schedule watchdog, a failed C call ...) must not leave the other ranks waiting:
        with several ranks its flag is set, the collective is joined, and then it is raised.  The caller reads the summed
        flags with whatever else it reads back (:meth:`_failed_elsewhere`)."""
        if self.world_size == 1:
            return share()
        failure = None
        try:
            share()
        except Exception as e:
            failure = e
            fused[-2 if isinstance(e, np.linalg.LinAlgError) else -1] = 1.0
        dist.allreduce_sum_(fused, self.group)
        if failure is not None:
            raise failure

    @staticmethod
    def _failed_elsewhere(flags, failed, not_pd=None):
        """Raise for the summed failure flags of :meth:`_sum_shares` (host values) set by another rank: RuntimeError
        ``failed``, or LinAlgError ``not_pd`` (if given) when only the not-positive-definite flag is set."""
        if flags[1] != 0.0 or (flags[0] != 0.0 and not_pd is None):
            raise RuntimeError(failed)
        if flags[0] != 0.0:
            raise np.linalg.LinAlgError(not_pd)

    def _predict(self, test_x, index_set, want_var, include_noise=True):
        xs = self._test_points(test_x)
        ns = xs.shape[0]
        layers = self._test_layers(index_set, ns, include_noise)
        if self.world_size > 1:
            return self._predict_ranks(xs, index_set, layers, want_var)
        # fused [mean | var] buffer
        fused = torch.zeros((self.dy + 1, ns), dtype=self.dtype, device=self.device)
        mean = torch.zeros((ns, self.dy), dtype=self.dtype, device=self.device)
        var = fused[self.dy] if want_var else None
        # blocks of a layer write disjoint test ranges: equal-sized ones in ONE batched call, the others in flight
        # together on the stream pool; layers accumulate into the same ranges and follow one another
        for j, bounds, add_noise, owned in layers:
            self.posterior_obj[j].predict_layer(self._x_dev, xs, bounds, owned, mean, var, add_noise)
        mean_np = mean.double().cpu().numpy()
        var_np = fused[self.dy].double().cpu().numpy() if want_var else None
        return mean_np, var_np

    def _predict_ranks(self, xs, index_set, layers, want_var):
        """:meth:`_predict` with several ranks: every serving layer has a zero [mean | var] slab of its own, into which
        this rank's blocks of that layer write; ONE collective sums the slabs over the ranks -- a test row of a layer is
        served by one block, so every element has one non-zero term and the sum is exact -- and the layers' slabs are then
        added in layer order, which is the order a single rank accumulates in: the prediction does not depend on the rank
        count or on ownership, bit for bit."""
        ns, q = xs.shape[0], self.dy
        serving = 1 if index_set is None else index_set.get_n_resolutions() + 1
        slab = ns * (q + 1)
        fused = torch.zeros(serving * slab, dtype=self.dtype, device=self.device)
        for j, bounds, add_noise, owned in layers:
            part = fused[j * slab:(j + 1) * slab]
            self.posterior_obj[j].predict_layer(self._x_dev, xs, bounds, owned, part[:ns * q].view(ns, q),
                                                part[ns * q:] if want_var else None, add_noise)
        dist.allreduce_sum_(fused, self.group)
        total = torch.zeros(slab, dtype=self.dtype, device=self.device)
        for j in range(serving):
            total = total + fused[j * slab:(j + 1) * slab]
        mean_np = total[:ns * q].view(ns, q).double().cpu().numpy()
        var_np = total[ns * q:].double().cpu().numpy() if want_var else None
        return mean_np, var_np

    def get_predicted_mean(self, test_x, index_set_obj=None, number_of_regions=None):
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        return self._predict(test_x, index_set_obj, want_var=False)[0]

    def get_central_moment2(self, test_x, index_set_obj=None, number_of_regions=None):
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        return self._predict(test_x, index_set_obj, want_var=True)[1]

    def get_predicted_mean_and_var(self, test_x, index_set_obj=None, number_of_regions=None, include_noise=True):
        """One pass for both moments (the reference needs two calls)."""
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        return self._predict(test_x, index_set_obj, want_var=True, include_noise=include_noise)

    # ------------------------------------------------------ predictive gradients
    def predictive_gradients(self, test_x, index_set_obj=None, number_of_regions=None):
        """Derivatives of the prediction with respect to the test inputs (GPy's ``GP.predictive_gradients``):
        ``(dmu_dx, dvar_dx)``, NumPy arrays of shape (N*, d, dy) and (N*, d), in the caller's original input units (the
        chain rule through ``standard_normalized_inputs``) and the output units of :meth:`get_predicted_mean_and_var`.
        Test point i is served by the blocks :meth:`_predict` gives it, so its gradient is the sum of theirs; biases and
        the finest layer's noise are constant.  The index-set rules and errors are those of :meth:`_predict`.  With
        several ranks every rank adds its blocks into one zero-initialised buffer, summed by ONE collective.  Not for
        ``adaptive_inputs`` (the warp's Jacobian is not built)."""
        if self.adaptive_inputs is True:
            raise TypeError('not yet supported')
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        self._refuse_sparse(index_set_obj)
        xs = self._test_points(test_x, index_set_obj, number_of_regions)
        ns, d = int(xs.shape[0]), int(xs.shape[1])
        q = self.dy
        fused = torch.zeros(ns * d * (q + 1), dtype=self.dtype, device=self.device)
        mean_grad = fused[:ns * d * q].view(ns, d, q)
        var_grad = fused[ns * d * q:].view(ns, d)
        for j, bounds, _, owned in self._test_layers(index_set_obj, ns):
            self.posterior_obj[j].predict_grad_layer(self._x_dev, xs, bounds, owned, mean_grad, var_grad)
        if self.world_size > 1:
            dist.allreduce_sum_(fused, self.group)
        dmu = mean_grad.double().cpu().numpy()
        dvar = var_grad.double().cpu().numpy()
        if self.standard_normalized_inputs is True:
            inv_std = 1.0 / np.asarray(self.std_x_train, dtype=np.float64)
            dmu = dmu * inv_std[None, :, None]
            dvar = dvar * inv_std[None, :]
        return dmu, dvar

    # ------------------------------------------------------- joint distribution
    def _joint(self, xs, index_set, include_noise, rows, sampling, seed=0, jitter=1e-6):
        """Every owned block's share of the (rows x N*) covariance or ``sampling`` buffer, summed over the ranks
        (:meth:`_sum_shares`); returns the buffer."""
        ns = xs.shape[0]
        fused = torch.zeros(rows * ns + 2, dtype=self.dtype, device=self.device)
        buf = fused[:rows * ns].view(rows, ns)
        self.last_joint_jitter = [0.0] * self.n_layers
        layers = self._test_layers(index_set, ns, include_noise)

        def share():
            for j, bounds, add_noise, owned in layers:
                self.last_joint_jitter[j] = self.posterior_obj[j].joint_layer(
                    j, self._x_dev, xs, bounds, owned, add_noise, None if sampling else buf, buf if sampling else None,
                    seed, jitter)

        self._sum_shares(fused, share)
        if self.world_size > 1:
            self._failed_elsewhere(fused[-2:].cpu().numpy(),
                                   'joint predictive distribution failed on another rank (see its exception)',
                                   'joint predictive covariance not positive definite (a block owned by another rank)')
        return buf

    def get_predicted_covariance(self, test_x, index_set_obj=None, number_of_regions=None, include_noise=True):
        """Joint predictive covariance (N* x N*, a symmetric NumPy array) of the latent function at ``test_x``, shared
        by all outputs: the sum over the layers of each region's K(X*, X*) - W W^T, W = K(X*, X) L^-T, entries between
        test points of different regions of a layer being 0.  ``include_noise``: the finest layer's block
        noise on the diagonal, as in :meth:`get_predicted_mean_and_var`, whose variance is this matrix's diagonal.
        Assembled on the device from the blocks' lower triangles: memory is N*^2 elements.  Not with a sparse layer among
        those that serve the test points."""
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        self._refuse_sparse(index_set_obj)
        xs = self._test_points(test_x, index_set_obj, number_of_regions)
        cov = self._joint(xs, index_set_obj, include_noise, xs.shape[0], sampling=False)
        cov = torch.tril(cov) + torch.tril(cov, -1).t()
        return cov.double().cpu().numpy()

    def posterior_samples(self, test_x, size=1, index_set_obj=None, number_of_regions=None, seed=0, include_noise=True,
                          jitter=1e-6):
        """``size`` draws (size, N*, dy) from the joint predictive distribution at ``test_x``: the predictive mean plus,
        per layer j and region l, chol(Sigma_jl + jitter sf2_j I) Z_jl with Z_jl[c][i] = phi(seed, j 2^32 + l, c, i),
        c = sample * dy + output (include/cimrgp_joint.h).  Outputs are independent; a request for fewer samples gives a
        prefix of a longer one, whatever the rank count.  A block whose factorisation fails is retried with 10x the
        jitter (at most 4 times), then numpy.linalg.LinAlgError names the layer and region;
        ``self.last_joint_jitter[j]``: the largest relative jitter the owned blocks of layer j needed.  Not with a sparse
        layer among those that serve the test points."""
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        self._refuse_sparse(index_set_obj)
        if index_set_obj is not None:
            self._check_index_set(index_set_obj, number_of_regions)
        if int(size) < 1:
            raise ValueError('size must be at least 1')
        if not (float(jitter) >= 0.0):
            raise ValueError('jitter must be non-negative')
        mean = self._predict(test_x, index_set_obj, want_var=False)[0]
        xs = self._test_points(test_x)
        size, ns = int(size), xs.shape[0]
        out = self._joint(xs, index_set_obj, include_noise, size * self.dy, True, int(seed), float(jitter))
        dev_part = out.double().cpu().numpy().reshape(size, self.dy, ns).transpose(0, 2, 1)
        return mean[None, :, :] + dev_part

    # ------------------------------------------------- leave-one-out cross-validation
    def leave_one_out(self, layer=None):
        """Leave-one-out prediction of every training target: ``(loo_mean (N, dy), loo_var (N,))``, NumPy arrays in the
        output units of :meth:`get_predicted_mean_and_var` ("Leave-one-out cross-validation").  For the block
        (``layer`` j, region l) that holds point i, with K = K_j(X, X) + noise I, alpha = K^-1 (y - f_bar_j - bias) and
        d = diag(K^-1):  loo_mean[i] = y[i] - alpha[i] / d_i,  loo_var[i] = 1 / d_i (noise included, shared by the
        outputs).  This is the BLOCKWISE leave-one-out of layer j conditional on the coarser layers: point i is withheld
        from its layer-j block only; the prediction f_bar_j of layers 0 .. j - 1, the block's bias and its noise are those
        of the fit and keep their dependence on y[i].  That is how the model is fitted and how its hyper-parameters are
        learned (layer by layer); it is not a refit of the whole chain.  ``layer=None``: the finest layer.  Closed form
        (Rasmussen & Williams 5.4.2): nothing is refitted, sampled or jittered.  Needs ``keep_factors=True``.  With
        several ranks every rank adds its blocks into one zero buffer, summed by ONE collective of [mean | var | failure
        flags]."""
        if not self._fitted:
            raise RuntimeError('call fit() before leave_one_out()')
        if not self.keep_factors:
            raise RuntimeError('leave-one-out needs the Cholesky factors: construct the model with keep_factors=True')
        j = self.n_layers - 1 if layer is None else int(layer)
        if not 0 <= j < self.n_layers:
            raise ValueError('layer must be in [0, %d), got %r' % (self.n_layers, layer))
        if self._is_sparse(j):
            raise TypeError('not yet supported')
        n, q = self._y.shape
        fused = torch.zeros(n * q + n + 2, dtype=self.dtype, device=self.device)
        mean, var = fused[:n * q].view(n, q), fused[n * q:n * q + n]
        self._sum_shares(fused, lambda: self.posterior_obj[j].loo_layer(self._y, self._slices(self._y, j), self._owned(j),
                                                                        mean, var))
        res = fused.double().cpu().numpy()
        self._failed_elsewhere(res[-2:], 'leave-one-out failed on another rank (see its exception)')
        return res[:n * q].reshape(n, q).copy(), res[n * q:n * q + n].copy()

    def get_loo_likelihood(self, layer=None):
        """:meth:`get_test_likelihood`'s formula (kept as it is, so that the two numbers are comparable) applied to the
        training targets and their leave-one-out predictions of ``layer`` (:meth:`leave_one_out`): a score that needs no
        held-out set."""
        mf, vf = self.leave_one_out(layer)
        ll = -0.5 * np.log(2 * np.pi * vf) - 0.5 * (np.linalg.norm((self.observations - mf), axis=1) ** 2) / vf
        return np.mean(ll)

    def get_test_likelihood(self, test, index_set_obj=None, number_of_regions=None):
        test_x, test_y = test[0], test[1]
        mf, vf = self.get_predicted_mean_and_var(test_x, index_set_obj, number_of_regions)
        ll = -0.5 * np.log(2 * np.pi * vf) - 0.5 * (np.linalg.norm((test_y - mf), axis=1) ** 2) / vf
        return np.mean(ll)

    @staticmethod
    def _compute_initial_noise_var_from_snr(y, snr_ratio):
        n_samps = y.shape[0]
        y_var = (np.linalg.norm(y) ** 2) / n_samps - np.dot(np.mean(y, axis=0), np.mean(y, axis=0))
        return y_var / snr_ratio
