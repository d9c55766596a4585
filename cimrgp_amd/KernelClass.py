"""Kernel / basis objects of the path.

``RBFKernel`` is the new covariance object of the dense path; it follows the
protocol of the reference's ``MaternKernel`` (KernelClass.py:40-65: attributes
``l``, ``sf``; methods ``kernel``, ``log_kernel``, ``spectral``,
``log_spectral``, ``estimate_kernel``) so that it can be passed as
``spectral_density_obj`` (scalar or per-layer list, MRGP.py:71-79), and adds
the Gram builder that runs on the GPU (``DeviceGram``, shared).  ``DenseMaternKernel`` is its Matern twin for
half-integer nu (1/2, 3/2, 5/2) in closed form: the prior that the reduced-rank
model approximates, on the same dense path.  ``MaternKernel`` and
``LaplacianEigenpairs`` are host-side restatements of the reference's
reduced-rank objects, kept for API completeness (validated against captured
reference outputs in tests/golden/kernel_objects.npz).
"""
import numpy as np
from scipy.special import kv, gammaln

#: most input dimensions the covariance kernels take, so the most length-scales of an ARD kernel (csrc/common.hpp MAXD)
MAXD = 8


def _lengthscale(l):
    """``(l, ard)`` of a constructor's ``l``: a scalar stays a float (isotropic); a sequence becomes a fresh float64
    (d,) array, one length-scale per input dimension (ARD), 1 <= d <= MAXD."""
    if np.ndim(l) == 0:
        if not l > 0:
            raise ValueError('length-scale must be positive')
        return float(l), False
    v = np.array(l, dtype=np.float64)
    if v.ndim != 1 or v.size < 1:
        raise ValueError('length-scales must be a scalar or a sequence of at least one number')
    if v.size > MAXD:
        raise ValueError('at most %d length-scales, got %d' % (MAXD, v.size))
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError('length-scale must be positive')
    return v, True


def _refuse_ard(kernel):
    """The scalar-distance protocol is a function of ONE distance: an ARD kernel has none."""
    if kernel.ard:
        raise TypeError('not yet supported')


def _unit_inputs(kernel, x, x2):
    """``(x, x2, l)`` for the Gram calls: as given with the kernel's ``l``, or, under ARD, divided by the length-scales
    (``Hyper.unit_lengthscale`` / ``scaled``) with l = 1.0."""
    if not kernel.ard:
        return x, x2, kernel.l
    from .Hyper import scaled, unit_lengthscale
    for v in (x, x2):
        if v is not None and int(v.shape[1]) != len(kernel.l):
            raise ValueError('inputs of dimension %d under %d length-scales' % (int(v.shape[1]), len(kernel.l)))
    scale, xs = unit_lengthscale(x, kernel.l)
    return xs, None if x2 is None else scaled(x2, scale), 1.0


class DeviceGram(object):
    """The dense Gram builder (device, HIP) of a covariance class with ``l``, ``sf``, ``ard`` and ``cov``, its covariance
    id of the C ABI: :class:`RBFKernel`'s and :class:`DenseMaternKernel`'s."""

    def gram(self, x, x2=None, diag_add=0.0, lower_only=False):
        """Gram matrix on the GPU (k_gram).  ``x``/``x2``: CUDA tensors (n x d).  Returns a
        torch view (n x n2) of the padded device buffer."""
        from . import device as dev
        x, x2, l = _unit_inputs(self, x, x2)
        if x2 is None:
            buf = dev.rbf_gram(x, l, self.sf, diag_add, lower_only, cov=self.cov)
            return buf[:x.shape[0], :x.shape[0]]
        buf = dev.rbf_cross(x, x2, l, self.sf, cov=self.cov)
        return buf[:x.shape[0], :x2.shape[0]]

    def K(self, x, x2=None, dtype='f64'):
        """NumPy in / NumPy out convenience around :meth:`gram` (computed on the GPU)."""
        from . import device as dev
        device = dev.require_gpu()
        tdt = dev.as_torch_dtype(dtype)
        xd = dev.to_device(np.atleast_2d(x), tdt, device)
        x2d = None if x2 is None else dev.to_device(np.atleast_2d(x2), tdt, device)
        return self.gram(xd, x2d).cpu().numpy()


class RBFKernel(DeviceGram):
    """k(r) = sf * exp(-r^2 / (2 l^2));  ``sf`` is the signal VARIANCE, as the
    reference's kernels multiply by ``sf`` directly (KernelClass.py:77).
    ``noise``: fixed Gaussian noise variance of the blocks using this kernel,
    or None for the plugin's rule 0.01 * var(targets) (RegressionInput.py:62).
    ``l``: a scalar (``l`` a float, ``ard`` False) or a sequence of 1 .. MAXD positive numbers, one length-scale per input
    dimension (``l`` a (d,) float64 array, ``ard`` True): k = sf * exp(-1/2 sum_k ((x_k - x'_k) / l_k)^2)."""
    name = 'RBF'

    def __init__(self, l=1., sf=1., noise=None):
        self.l, self.ard = _lengthscale(l)
        if not sf > 0:
            raise ValueError('signal variance must be positive')
        self.sf = float(sf)
        self.noise = None if noise is None else float(noise)

    #: covariance id of the C ABI (include/cimrgp.h CIMRGP_COV_RBF)
    cov = 0

    def with_noise(self, noise):
        """The same covariance with fixed noise variance ``noise``."""
        return RBFKernel(self.l, self.sf, noise)

    def with_values(self, l, sf, noise):
        """The same covariance class with other values."""
        return RBFKernel(l, sf, noise)

    # ---- scalar-distance protocol (host, NumPy) ---------------------------
    def log_kernel(self, r):
        _refuse_ard(self)
        r = np.asarray(r, dtype=np.float64)
        return np.log(self.sf) - 0.5 * (r / self.l) ** 2

    def kernel(self, r):
        return np.exp(self.log_kernel(r))

    def log_spectral(self, s):
        # 1-D spectral density in the reference's convention (KernelClass.py:80-90):
        # S(s) = sf * sqrt(2 pi) * l * exp(-l^2 s^2 / 2)
        _refuse_ard(self)
        s = np.asarray(s, dtype=np.float64)
        return np.log(self.sf) + 0.5 * np.log(2 * np.pi) + np.log(self.l) - 0.5 * (self.l * s) ** 2

    def spectral(self, s):
        return np.exp(self.log_spectral(s))

    def estimate_kernel(self, phi_x1, phi_x2, lambdas):
        """Reduced-rank reconstruction sum_p S(sqrt(lambda_p)) phi_p(x) phi_p(x')."""
        weights = self.spectral(np.sqrt(np.asarray(lambdas, dtype=np.float64)))
        return np.einsum('np,np,p->n', phi_x1, phi_x2, weights)


class LaplacianEigenpairs(object):
    """Dirichlet-Laplacian eigenpairs on [-L, L]^d (reference KernelClass.py:6-37):
    phi(x) = prod_k L_k^-1/2 sin(pi j (x_k + L_k) / (2 L_k)),  lambda = sum_k (pi j / 2 L_k)^2."""
    name = 'Laplacian'

    def get_eigenpairs(self, x, basis_id, basis_interval=None, per_dimension=False):
        x = np.asarray(x)
        if basis_interval is None:
            basis_interval = np.max(np.abs(x), axis=0)
        basis_interval = np.asarray(basis_interval, dtype=np.float64)
        if len(basis_interval) != x.shape[1]:
            raise ValueError('Basis interval should have the same dimensionality as the input.')
        phi, lam = self._learn(x, basis_interval, basis_id)
        if per_dimension is True:
            return phi, lam
        return np.prod(phi, axis=1), np.sum(lam)

    @staticmethod
    def _learn(x, basis_interval, basis_id):
        half = basis_interval[None, :]
        phi = np.sin((np.pi * basis_id) * (x + half) / (2 * half)) / np.sqrt(half)
        lam = ((np.pi * basis_id) / (2 * basis_interval)) ** 2
        return phi, lam


class MaternKernel(object):
    """Matern covariance of a scalar distance and its spectral density, in the log
    domain (reference KernelClass.py:40-90)."""
    name = 'Matern'

    def __init__(self, nu=1, l=1, sf=1):
        self.nu = nu
        self.l = l
        self.sf = sf

    def log_kernel(self, r):
        nu, ell = self.nu, self.l
        log_arg = np.log(np.sqrt(2 * nu) * r) - np.log(ell)
        return (np.log(self.sf) + (1 - nu) * np.log(2) - gammaln(nu) + nu * log_arg
                + np.log(kv(nu, np.exp(log_arg))))

    def kernel(self, r):
        return np.exp(self.log_kernel(r))

    def log_spectral(self, s):
        nu, ell = self.nu, self.l
        log_arg = np.log(2 * nu) - 2 * np.log(ell)
        return (np.log(self.sf) + 0.5 * np.log(2 * np.pi) + nu * log_arg + gammaln(nu + 0.5) - gammaln(nu)
                - (nu + .5) * np.log(np.exp(log_arg) + np.asarray(s) ** 2))

    def spectral(self, s):
        return np.exp(self.log_spectral(s))

    def estimate_kernel(self, phi_x1, phi_x2, lambdas):
        weights = self.spectral(np.sqrt(np.asarray(lambdas, dtype=np.float64)))
        return np.einsum('np,np,p->n', phi_x1, phi_x2, weights)


class DenseMaternKernel(DeviceGram):
    """Matern covariance of half-integer smoothness on the dense path, in closed form with
    t = sqrt(2 nu) r / l:
        nu = 1/2:  sf exp(-t)                  (the exponential covariance)
        nu = 3/2:  sf (1 + t) exp(-t)          (GPy's Matern32(variance=sf, lengthscale=l))
        nu = 5/2:  sf (1 + t + t^2 / 3) exp(-t) (GPy's Matern52)
    ``sf`` is the signal VARIANCE and k(0) = sf, as for :class:`RBFKernel`, whose protocol this
    follows; ``spectral`` / ``estimate_kernel`` are those of :class:`MaternKernel` (the reference's
    convention), so that the reduced-rank model over the Laplacian basis converges to this kernel
    up to the reference's factor sqrt(2).  General real nu stays with :class:`MaternKernel`.
    ``l``: a scalar, or a sequence of per-dimension length-scales (ARD) as for :class:`RBFKernel`: r is then
    sqrt(sum_k ((x_k - x'_k) / l_k)^2) at l = 1."""
    name = 'Matern'
    #: nu -> covariance id of the C ABI (include/cimrgp.h CIMRGP_COV_MATERN12/32/52)
    COV_IDS = {0.5: 1, 1.5: 2, 2.5: 3}

    def __init__(self, nu=1.5, l=1., sf=1., noise=None):
        if float(nu) not in self.COV_IDS:
            raise ValueError('nu must be 0.5, 1.5 or 2.5 (general nu: MaternKernel, reduced-rank path only)')
        self.l, self.ard = _lengthscale(l)
        if not sf > 0:
            raise ValueError('signal variance must be positive')
        self.nu = float(nu)
        self.sf = float(sf)
        self.noise = None if noise is None else float(noise)
        self.cov = self.COV_IDS[self.nu]

    def with_noise(self, noise):
        """The same covariance with fixed noise variance ``noise``."""
        return DenseMaternKernel(self.nu, self.l, self.sf, noise)

    def with_values(self, l, sf, noise):
        """The same covariance class (and nu) with other values."""
        return DenseMaternKernel(self.nu, l, sf, noise)

    # ---- scalar-distance protocol (host, NumPy) ---------------------------
    def _log_poly(self, t):
        if self.nu == 0.5:
            return np.zeros_like(t)
        if self.nu == 1.5:
            return np.log1p(t)
        return np.log1p(t + t * t / 3.0)

    def log_kernel(self, r):
        _refuse_ard(self)
        t = np.sqrt(2 * self.nu) * np.abs(np.asarray(r, dtype=np.float64)) / self.l
        return np.log(self.sf) + self._log_poly(t) - t

    def kernel(self, r):
        return np.exp(self.log_kernel(r))

    def _matern(self):
        _refuse_ard(self)
        return MaternKernel(nu=self.nu, l=self.l, sf=self.sf)

    def log_spectral(self, s):
        return self._matern().log_spectral(s)

    def spectral(self, s):
        return self._matern().spectral(s)

    def estimate_kernel(self, phi_x1, phi_x2, lambdas):
        """Reduced-rank reconstruction sum_p S(sqrt(lambda_p)) phi_p(x) phi_p(x')."""
        return self._matern().estimate_kernel(phi_x1, phi_x2, lambdas)


class SparseKernel(object):
    """Marks a layer of ``MultiResolutionGaussianProcess`` as SPARSE: its blocks are inducing-point GPs (``Sparse.SparseBlock``,
    FITC or VFE / DTC) under the wrapped covariance ``kernel`` (an :class:`RBFKernel` or a :class:`DenseMaternKernel`),
    n m^2 flop and n m memory per block instead of n^3 / 3 and n^2 ("Sparse layers in the multiresolution
    model").  ``l``, ``sf``, ``noise``, ``cov`` and ``nu`` are the wrapped kernel's.

    A region of n rows gets m = min(n, ``num_inducing``) inducing inputs, rows of the region's own (normalised, warped)
    inputs picked by ``inducing``: ``'stride'`` -- rows floor((k + 0.5) n / m), k = 0 .. m - 1 (every row, in order, when
    m = n) -- or ``'random'`` -- ``numpy.random.RandomState([seed, layer, region]).permutation(n)[:m]``.  Either is a
    function of (seed, layer, region, n) alone.  ``'greedy'`` picks the m rows of largest conditional variance under the
    wrapped kernel as the layer was constructed (``Inducing.greedy_rows``; DESIGN.md, "Greedy inducing-point selection"): a
    function of the region's inputs and that kernel alone, made once per region on the device and kept, so
    ``Sparse.SparsePosterior.inducing_rows`` has them and :meth:`inducing_rows`, which has no data, does not.
    ``jitter``: eps of K_uu + eps sf I.  ``ard`` is the wrapped kernel's too:
    a base with per-dimension length-scales makes an ARD sparse layer."""
    INDUCING = ('stride', 'random', 'greedy')

    def __init__(self, kernel, num_inducing=1000, approximation='fitc', jitter=1e-6, inducing='stride', seed=0):
        from .Sparse import APPROXIMATIONS
        if not isinstance(kernel, (RBFKernel, DenseMaternKernel)):
            raise TypeError('SparseKernel wraps an RBFKernel or a DenseMaternKernel, got %s' % type(kernel).__name__)
        if int(num_inducing) < 1:
            raise ValueError('num_inducing must be at least 1')
        if str(approximation).lower() not in APPROXIMATIONS:
            raise ValueError("approximation must be one of %s, got %r" % (sorted(APPROXIMATIONS), approximation))
        if not float(jitter) >= 0:
            raise ValueError('jitter must not be negative')
        if inducing not in self.INDUCING:
            raise ValueError("inducing must be 'stride', 'random' or 'greedy', got %r" % (inducing,))
        self.kernel = kernel
        self.num_inducing = int(num_inducing)
        self.approximation = str(approximation).lower()
        self.jitter = float(jitter)
        self.inducing = inducing
        self.seed = int(seed)

    name = 'Sparse'

    l = property(lambda self: self.kernel.l)
    sf = property(lambda self: self.kernel.sf)
    noise = property(lambda self: self.kernel.noise)
    cov = property(lambda self: self.kernel.cov)
    ard = property(lambda self: self.kernel.ard)

    @property
    def nu(self):
        return self.kernel.nu          # AttributeError for an RBF base, as on the base itself

    def rewrap(self, kernel):
        """A SparseKernel with these settings around another base kernel."""
        return SparseKernel(kernel, self.num_inducing, self.approximation, self.jitter, self.inducing, self.seed)

    def with_noise(self, noise):
        """The same sparse layer with fixed noise variance ``noise``."""
        return self.rewrap(self.kernel.with_noise(noise))

    def with_values(self, l, sf, noise):
        """The same sparse layer around the base covariance with other values."""
        return self.rewrap(self.kernel.with_values(l, sf, noise))

    def inducing_rows(self, layer, region, n):
        """Row numbers (int64, length min(n, num_inducing)) of the inducing inputs of region ``region`` of layer ``layer``
        with ``n`` rows.  ``'greedy'`` rows depend on the region's inputs, which this object never sees: TypeError."""
        if self.inducing == 'greedy':
            raise TypeError("the rows of inducing='greedy' are a function of the region's inputs: "
                            "ask SparsePosterior.inducing_rows(region) after the fit")
        n = int(n)
        m = min(n, self.num_inducing)
        if self.inducing == 'stride':
            return ((2 * np.arange(m, dtype=np.int64) + 1) * n) // (2 * m)
        return np.random.RandomState([self.seed, int(layer), int(region)]).permutation(n)[:m].astype(np.int64)
