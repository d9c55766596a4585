"""NumPy restatement of the multiresolution model with sparse (inducing-point) layers ("Sparse layers in the
multiresolution model"), shared by tests/test_sparse_layer_host.py and the GPU tests.  The coarse-to-fine residual chain of
oracle/mrgp.py with each block either exact (sparse_numpy.exact) or sparse; the sparse blocks are written twice over:
``form='woodbury'`` takes them from sparse_numpy.woodbury (the chain the device runs), ``form='dense'`` from
sparse_numpy.dense (the n x n definition).  Bias and noise follow DenseBlock.fit: bias = column means of the block's
residual targets (or the layer's), noise = the kernel's, else max(0.01 x pooled population variance, 1e-8 sf) of the
block (or of the layer).  Covariance ids are those of include/cimrgp.h; mode 0 = FITC, 1 = VFE."""
import numpy as np

import sparse_numpy as sn
import sparse_grad_numpy as sg

NOISE_FRACTION, NOISE_FLOOR = 0.01, 1e-8


class Layer(object):
    """One resolution: covariance (cov, ell, sf2), fixed noise or None, and for a sparse layer m = num_inducing, mode,
    eps = jitter, the inducing rule and its seed (m None: an exact layer)."""

    def __init__(self, cov, ell, sf2=1.0, noise=None, m=None, mode=0, eps=1e-6, inducing='stride', seed=0):
        self.cov, self.ell, self.sf2, self.noise = cov, ell, sf2, noise
        self.m, self.mode, self.eps, self.inducing, self.seed = m, mode, eps, inducing, seed


def stride_rows(n, m):
    """Rows floor((k + 0.5) n / m), k = 0 .. m - 1, of a region of n rows (m <= n), in exact integer arithmetic."""
    return np.array([((2 * k + 1) * n) // (2 * m) for k in range(m)], dtype=np.int64)


def inducing_rows(layer, j, l, n):
    m = min(n, layer.m)
    if layer.inducing == 'stride':
        return stride_rows(n, m)
    return np.random.RandomState([layer.seed, j, l]).permutation(n)[:m]


def _noise_rule(r, layer):
    pooled = float(np.mean((r - r.mean(axis=0)) ** 2))
    return max(NOISE_FRACTION * pooled, NOISE_FLOOR * layer.sf2)


def _block(x, z, rc, layer, noise, xs, form):
    """(mean, latent var) of one block at xs."""
    if layer.m is None:
        _, mean, var = sn.exact(x, rc, layer.cov, layer.ell, layer.sf2, noise, xs)
        return mean, var
    f = sn.woodbury if form == 'woodbury' else sn.dense
    _, mean, var = f(x, z, rc, layer.cov, layer.ell, layer.sf2, noise, layer.eps, layer.mode, xs)
    return mean, var


def chain(x, y, bounds, layers, xs=None, test_bounds=None, include_noise=True, form='woodbury', bias_region_specific=True,
          noise_region_specific=True):
    """One coarse-to-fine sweep over ``bounds`` (a list over layers of lists of (a, b) row ranges of the normalised inputs
    ``x``) and the prediction at ``xs`` (test block (j, l) = rows test_bounds[j][l], served by training block (j, l); the
    finest layer of ``test_bounds`` adds its blocks' noise with ``include_noise``).  Returns a dict: f_bar (N x q, the sum
    of all layers at the training points), f_bar_layers (what layer j was fitted against), mean / var (None without xs),
    blocks[j][l] = dict(bias, noise, rows)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    q = y.shape[1]
    f_bar = np.zeros_like(y)
    ns = 0 if xs is None else xs.shape[0]
    mean, var = (np.zeros((ns, q)), np.zeros(ns)) if xs is not None else (None, None)
    n_test_layers = 0 if xs is None else len(test_bounds)
    blocks, f_bar_layers = [], []
    for j, layer in enumerate(layers):
        resid = y - f_bar
        f_bar_layers.append(f_bar)
        shared_bias = resid.mean(axis=0)
        shared_noise = _noise_rule(resid, layer)
        mu = np.zeros_like(y)
        row = []
        for l, (a, b) in enumerate(bounds[j]):
            a, b = int(a), int(b)
            r = resid[a:b]
            bias = r.mean(axis=0) if bias_region_specific else shared_bias
            if layer.noise is not None:
                noise = float(layer.noise)
            else:
                noise = _noise_rule(r, layer) if noise_region_specific else shared_noise
            rc = r - bias
            xb = x[a:b]
            rows = None if layer.m is None else inducing_rows(layer, j, l, b - a)
            z = None if rows is None else xb[rows]
            ta, tb = (int(v) for v in test_bounds[j][l]) if j < n_test_layers else (0, 0)
            at = xb if tb <= ta else np.concatenate([xb, xs[ta:tb]])
            m_all, v_all = _block(xb, z, rc, layer, noise, at, form)
            mu[a:b] = m_all[:b - a] + bias
            if tb > ta:
                mean[ta:tb] += m_all[b - a:] + bias
                var[ta:tb] += v_all[b - a:]
                if include_noise and j == n_test_layers - 1:
                    var[ta:tb] += noise
            row.append(dict(bias=bias, noise=noise, rows=rows))
        blocks.append(row)
        f_bar = f_bar + mu
    return dict(f_bar=f_bar, f_bar_layers=f_bar_layers, mean=mean, var=var, blocks=blocks)


def gap(a, b):
    """Largest gaps between two chains: (mean, var, f_bar); mean / var None without test points."""
    g = lambda u, v: None if u is None else float(np.abs(u - v).max())
    return g(a['mean'], b['mean']), g(a['var'], b['var']), g(a['f_bar'], b['f_bar'])


def tolerance(a, b):
    """The project's rule (tests/test_gpu_sparse.py, _tolerance): 100 x the largest gap between the two NumPy forms on the
    same inputs, floor 1e-9, for (mean, var, f_bar)."""
    return tuple(None if g is None else max(1e-9, 100.0 * g) for g in gap(a, b))


def layer_objective(x, resid, bounds_j, layer, j, ell, sf2, noise, bias_region_specific=True):
    """Sum over the regions of layer j of the sparse objective and its gradient w.r.t. (log sf2, log ell, log noise) at
    (ell, sf2, noise) on the residual targets ``resid`` = y - f_bar_j, Z by the layer's rule: ((lml, grad) by
    sparse_grad_numpy.chain, (lml, grad) by sparse_grad_numpy.autograd of the restated chain)."""
    out = []
    for f in (lambda *a: sg.chain(*a)[:2], lambda *a: sg.autograd(*a, want_z=False)[:2]):
        lml, grad = 0.0, np.zeros(3)
        for l, (a, b) in enumerate(bounds_j):
            a, b = int(a), int(b)
            r = resid[a:b]
            rc = r - (r.mean(axis=0) if bias_region_specific else resid.mean(axis=0))
            z = x[a:b][inducing_rows(layer, j, l, b - a)]
            v, g = f(x[a:b], z, rc, layer.cov, ell, sf2, noise, layer.eps, layer.mode)
            lml, grad = lml + float(v), grad + np.asarray(g, dtype=np.float64)
        out.append((lml, grad))
    return out


def problem(n, d, ns, seed, repeat=False):
    """The issue's inputs: x uniform on [-2, 2]^d sorted by the first coordinate (``repeat``: every row twice), q = 2 smooth
    targets plus noise, ns test points sorted likewise."""
    rng = np.random.default_rng(seed)

    def draw(k):
        u = rng.uniform(-2, 2, size=(k, d))
        return u[np.argsort(u[:, 0], kind='stable')]

    if repeat:
        x = np.repeat(draw((n + 1) // 2), 2, axis=0)[:n]
    else:
        x = draw(n)
    y = np.stack([np.sin(2 * x).sum(axis=1), np.cos(x).prod(axis=1)], axis=1) + 0.1 * rng.normal(size=(n, 2))
    xs = draw(ns)
    ys = np.stack([np.sin(2 * xs).sum(axis=1), np.cos(xs).prod(axis=1)], axis=1) + 0.1 * rng.normal(size=(ns, 2))
    return x, y, xs, ys


def normalise(x, xs):
    mu, sd = x.mean(axis=0), x.std(axis=0)
    return (x - mu) / sd, (xs - mu) / sd


# ---- the shapes of the checks: N = 2801, divider 2, two resolutions -> regions of 2801 / 1400, 1401 / 700, 700, 700, 701 rows
# (ragged, two sizes per layer); m = 130 = two 128-column tiles, the second ragged; q = 2; 701 test points ------------------
N, NS, RES, DIVIDER, M = 2801, 701, 2, 2, 130
ELLS = (1.0, 0.5, 0.25)
_CHAINS = {}


def index_bounds(n):
    from cimrgp_amd import IndexSetUniform
    return [[(int(a), int(b)) for a, b in layer] for layer in IndexSetUniform(n, RES, DIVIDER).bounds]


def case_layers(cov, mode, sparse=(0, 1), inducing='stride', m=M, eps=1e-6, noise=None):
    return [Layer(cov, ELLS[j], 1.0, noise, m if j in sparse else None, mode, eps, inducing, seed=3) for j in range(RES + 1)]


def case_chain(d, cov, mode, sparse=(0, 1), inducing='stride', form='woodbury', m=M, eps=1e-6, noise=None, include_noise=True,
               bias_region_specific=True, noise_region_specific=True, seed=0):
    """The chain of one case on problem(N, d, NS, seed), computed once per process and shared (never modified)."""
    key = (d, cov, mode, tuple(sparse), inducing, form, m, eps, noise, include_noise, bias_region_specific, noise_region_specific,
           seed)
    if key not in _CHAINS:
        x, y, xs, _ = problem(N, d, NS, seed)
        xn, xsn = normalise(x, xs)
        _CHAINS[key] = chain(xn, y, index_bounds(N), case_layers(cov, mode, sparse, inducing, m, eps, noise), xsn, index_bounds(NS),
                             include_noise, form, bias_region_specific, noise_region_specific)
    return _CHAINS[key]
