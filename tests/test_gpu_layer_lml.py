"""The batched layer objective (cimrgp_layer_lml_grad_cov) against NumPy / SciPy, and the model's per-layer
hyper-parameter learning (MultiResolutionGaussianProcess(optimize_hyperparameters=True)) against a NumPy driver of the
same L-BFGS-B over the oracle's objective."""
import os

import numpy as np
import pytest
import scipy.linalg as sla

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COVS = {0: None, 1: 0.5, 2: 1.5, 3: 2.5}        # CIMRGP_COV_* -> Matern nu (None: RBF)


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


# ---- NumPy restatement ---------------------------------------------------------------------
def _cov(xa, xb, cov, ell, sf2):
    """k and d k / d log ell."""
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    if COVS[cov] is None:
        k = sf2 * np.exp(-0.5 * d2 / ell ** 2)
        return k, k * d2 / ell ** 2
    nu = COVS[cov]
    t = np.sqrt(2 * nu) * np.sqrt(d2) / ell
    v = np.exp(-t)
    if nu == 0.5:
        return sf2 * v, sf2 * t * v
    if nu == 1.5:
        return sf2 * (1 + t) * v, sf2 * t * t * v
    return sf2 * (1 + t + t * t / 3) * v, sf2 * t * t * (1 + t) * v / 3


def np_lml_grad(x, r, cov, ell, sf2, noise):
    """LML of targets r (n x q) and its gradient w.r.t. (log sf2, log ell, log noise): the oracle for the RBF, the same
    formulas restated here for the Matern covariances."""
    if COVS[cov] is None:
        return oracle.mrgp.gp_lml_and_grad(x, r, ell, sf2, noise)
    n, q = r.shape
    k, dk = _cov(x, x, cov, ell, sf2)
    chol = sla.cholesky(k + noise * np.eye(n), lower=True)
    alpha = sla.cho_solve((chol, True), r)
    lml = -0.5 * np.sum(r * alpha) - q * np.sum(np.log(np.diag(chol))) - 0.5 * n * q * np.log(2 * np.pi)
    g = alpha @ alpha.T - q * sla.cho_solve((chol, True), np.eye(n))
    return lml, np.array([0.5 * np.sum(g * k), 0.5 * np.sum(g * dk), 0.5 * noise * np.trace(g)])


# ---- the entry point -----------------------------------------------------------------------
def _layer(rng, batch, n, d, q, gap=3, lead=5):
    rows = lead + batch * (n + gap)
    x = rng.uniform(-2, 2, size=(rows, d))
    y = np.stack([np.sin(2 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(q)], axis=1) + 0.1 * rng.normal(size=(rows, q)) + 0.5
    fbar = 0.3 * rng.normal(size=(rows, q))
    starts = [lead + b * (n + gap) for b in range(batch)]
    return x, y, fbar, starts


def _run(ca, x, y, fbar, starts, n, cov, ell, sf2, noise, shared_bias=None, dtype=torch.float64):
    dev = ca.device
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
    batch = len(starts)
    ld = dev.padded_ld(n)
    ws_bytes = max((dev.potrf_workspace_bytes(n, dtype) + 15) // 16 * 16, 16)
    karena = torch.empty((batch, n, ld), dtype=dtype, device="cuda")
    kinv = torch.empty((batch, n, ld), dtype=dtype, device="cuda")
    ws = torch.empty((batch, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((batch, 4), np.nan, dtype=torch.float64, device="cuda")
    st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    dev.layer_lml_grad(t(x), t(y), t(fbar), st, n, ell, sf2, noise, t(shared_bias), karena, kinv, ws, info, out, cov=cov)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def _want(x, y, fbar, starts, n, cov, ell, sf2, noise, shared_bias=None):
    res = []
    for s in starts:
        r = y[s:s + n] - (0.0 if fbar is None else fbar[s:s + n])
        r = r - (r.mean(axis=0) if shared_bias is None else shared_bias)
        lml, g = np_lml_grad(x[s:s + n], r, cov, ell, sf2, noise)
        res.append([lml] + list(g))
    return np.asarray(res)


CASES = [  # batch, n, d, q, with fbar, shared bias
    (1, 65, 1, 2, True, False),
    (3, 256, 2, 3, False, True),
    (5, 300, 1, 3, True, True),
    (3, 1025, 2, 2, True, False),
    (5, 65, 2, 2, False, False),
    (1, 300, 2, 2, True, True),
]


@pytest.mark.parametrize("batch,n,d,q,with_fbar,shared", CASES)
def test_layer_lml_grad_matches_numpy(ca, batch, n, d, q, with_fbar, shared):
    rng = np.random.default_rng(1000 * batch + n)
    x, y, fbar, starts = _layer(rng, batch, n, d, q)
    fbar = fbar if with_fbar else None
    sb = np.array([0.4, -0.2, 0.1][:q]) if shared else None
    for cov in COVS:
        got, info = _run(ca, x, y, fbar, starts, n, cov, 0.7, 1.3, 0.05, sb)
        want = _want(x, y, fbar, starts, n, cov, 0.7, 1.3, 0.05, sb)
        assert np.all(info == 0), (cov, info)
        assert np.max(np.abs(got[:, 0] - want[:, 0]) / np.abs(want[:, 0])) < 1e-9, cov
        for b in range(batch):
            assert _rel(got[b, 1:], want[b, 1:]) < 1e-7, (cov, b)


def test_layer_lml_grad_matches_finite_differences(ca):
    rng = np.random.default_rng(7)
    n = 200
    x, y, fbar, starts = _layer(rng, 2, n, 2, 2)
    th = np.log([1.1, 0.6, 0.08])                  # (sf2, ell, noise)
    for cov in COVS:
        f = lambda t: _run(ca, x, y, fbar, starts, n, cov, np.exp(t[1]), np.exp(t[0]), np.exp(t[2]))[0]
        g = f(th)[:, 1:]
        for i in range(3):
            h = 1e-5
            e = np.zeros(3)
            e[i] = h
            fd = (f(th + e)[:, 0] - f(th - e)[:, 0]) / (2 * h)
            assert np.max(np.abs(fd - g[:, i]) / (np.abs(g[:, i]) + 1e-3)) < 1e-5, (cov, i)


def test_non_pd_block_leaves_the_others_intact(ca):
    rng = np.random.default_rng(3)
    n = 65
    x, y, fbar, starts = _layer(rng, 3, n, 1, 2)
    for s in starts:                               # well-spread inputs: the exponential covariance is PD without noise
        x[s:s + n, 0] = np.linspace(-2, 2, n) + 0.01 * rng.uniform(size=n)
    x[starts[1]:starts[1] + n, 0] = 0.25           # block 1: every input the same
    got, info = _run(ca, x, y, fbar, starts, n, 1, 0.5, 1.0, 0.0)
    assert info[1] > 0 and info[0] == 0 and info[2] == 0
    want = _want(x, y, fbar, [starts[0], starts[2]], n, 1, 0.5, 1.0, 0.0)
    for i, b in enumerate((0, 2)):
        assert abs(got[b, 0] - want[i, 0]) / abs(want[i, 0]) < 1e-9
        assert _rel(got[b, 1:], want[i, 1:]) < 1e-7


def test_fp32_agrees_with_fp64(ca):
    rng = np.random.default_rng(11)
    n = 128
    x, y, fbar, starts = _layer(rng, 3, n, 2, 2)
    for cov in COVS:
        g64, i64 = _run(ca, x, y, fbar, starts, n, cov, 0.8, 1.0, 0.2)
        g32, i32 = _run(ca, x, y, fbar, starts, n, cov, 0.8, 1.0, 0.2, dtype=torch.float32)
        assert np.all(i32 == 0) and np.all(i64 == 0)
        assert np.max(np.abs(g32[:, 0] - g64[:, 0]) / np.abs(g64[:, 0])) < 1e-3, cov
        for b in range(3):
            assert _rel(g32[b, 1:], g64[b, 1:]) < 1e-3, (cov, b)


# ---- the model -----------------------------------------------------------------------------
def _data(n=2001, ns=301, seed=5):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-2, 2, size=(n, 1)), axis=0)
    y = np.hstack([np.sin(3 * x) + 0.5 * np.sin(11 * x), np.cos(5 * x) * x]) + 0.1 * rng.normal(size=(n, 2))
    xs = np.sort(rng.uniform(-2, 2, size=(ns, 1)), axis=0)
    return x, y, xs


def _np_fit_predict(xn, y, bounds, layers, xsn, tbounds):
    """The dense MRGP (oracle.mrgp_fit / mrgp_predict) for any covariance: layers = [(cov, ell, sf2, noise)]."""
    f_bar = np.zeros_like(y)
    mean, var = np.zeros((xsn.shape[0], y.shape[1])), np.zeros(xsn.shape[0])
    for j, (cov, ell, sf2, noise) in enumerate(layers):
        mu = np.zeros_like(y)
        for (a, b), (ta, tb) in zip(bounds[j], tbounds[j]):
            r = y[a:b] - f_bar[a:b]
            bias = r.mean(axis=0)
            k, _ = _cov(xn[a:b], xn[a:b], cov, ell, sf2)
            chol = sla.cholesky(k + noise * np.eye(b - a), lower=True)
            alpha = sla.cho_solve((chol, True), r - bias)
            mu[a:b] = r - bias - noise * alpha + bias
            ks, _ = _cov(xsn[ta:tb], xn[a:b], cov, ell, sf2)
            mean[ta:tb] += ks @ alpha + bias
            w = sla.solve_triangular(chol, ks.T, lower=True)
            var[ta:tb] += sf2 - np.sum(w * w, axis=0) + (noise if j == len(layers) - 1 else 0.0)
        f_bar = f_bar + mu
    return mean, var


def _np_learn(xn, y, bounds, starts, max_iters=1000):
    """The NumPy driver: per layer, coarse to fine, L-BFGS-B on -sum_l LML_l of the residual targets (per-region
    bias), then the layer fitted with the learned values.  starts = [(cov, l, sf)] of the constructor's kernels."""
    from scipy.optimize import minimize
    layers, results = [], []
    for j, (cov, l0, sf0) in enumerate(starts):
        f_bar = np.zeros_like(y)
        if layers:
            f_bar = _fbar(xn, y, bounds, layers)

        def objective(theta):
            sf2, ell, noise = np.exp(theta)
            lml, grad = 0.0, np.zeros(3)
            for a, b in bounds[j]:
                r = y[a:b] - f_bar[a:b]
                try:
                    v, g = np_lml_grad(xn[a:b], r - r.mean(axis=0), cov, ell, sf2, noise)
                except np.linalg.LinAlgError:
                    return 1e100, np.zeros(3)
                lml, grad = lml + v, grad + g
            return -lml, -grad

        res = minimize(objective, np.log([sf0, l0, 0.01 * sf0]), jac=True, method='L-BFGS-B',
                       options=dict(maxiter=max_iters))
        sf2, ell, noise = np.exp(res.x)
        layers.append((cov, ell, sf2, noise))
        results.append(res)
    return layers, results


def _fbar(xn, y, bounds, layers):
    f_bar = np.zeros_like(y)
    for j, (cov, ell, sf2, noise) in enumerate(layers):
        mu = np.zeros_like(y)
        for a, b in bounds[j]:
            r = y[a:b] - f_bar[a:b]
            bias = r.mean(axis=0)
            k, _ = _cov(xn[a:b], xn[a:b], cov, ell, sf2)
            alpha = sla.cho_solve((sla.cholesky(k + noise * np.eye(b - a), lower=True), True), r - bias)
            mu[a:b] = r - noise * alpha
        f_bar = f_bar + mu
    return f_bar


def _kernels(ca, covs, res):
    ks = []
    for j in range(res + 1):
        l = 1.0 / 2 ** j
        ks.append(ca.RBFKernel(l=l, sf=1.0) if covs[j] == 0 else ca.DenseMaternKernel(COVS[covs[j]], l=l, sf=1.0))
    return ks


@pytest.mark.parametrize("covs", [(0, 0, 0, 0), (0, 2, 0, 2)])
def test_model_learns_what_the_numpy_driver_learns(ca, covs):
    x, y, xs = _data()
    n, ns, res = x.shape[0], xs.shape[0], 3
    kernels = _kernels(ca, covs, res)
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2), spectral_density_obj=kernels,
                                              optimize_hyperparameters=True)
    model.fit()
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(ns, res, 2))
    xn, _, mu, sd = oracle.normalize_inputs(x)
    bounds = oracle.index_bounds_uniform(n, res, 2)
    assert bounds[-1][-1][1] - bounds[-1][-1][0] != bounds[-1][0][1] - bounds[-1][0][0]    # a ragged last region
    layers, results = _np_learn(xn, y, bounds, [(covs[j], 1.0 / 2 ** j, 1.0) for j in range(res + 1)])
    for j in range(res + 1):
        k = model.posterior_obj[j].kernel
        assert k is not kernels[j] and type(k) is type(kernels[j])
        assert kernels[j].noise is None and kernels[j].l == 1.0 / 2 ** j        # the caller's objects are untouched
        _, ell, sf2, noise = layers[j]
        np.testing.assert_allclose([k.sf, k.l, k.noise], [sf2, ell, noise], rtol=1e-5)
        assert abs(model.optimizer_results[j].fun - results[j].fun) < 1e-8 * abs(results[j].fun)
    tb = oracle.index_bounds_uniform(ns, res, 2)
    if covs == (0, 0, 0, 0):
        specs = [oracle.DenseLayerSpec(ell, sf2, noise) for _, ell, sf2, noise in layers]
        omodel, _ = oracle.mrgp_fit(xn, y, bounds, specs)
        omean, ovar = oracle.mrgp_predict(xn, omodel, specs, (xs - mu) / sd, tb)
    else:
        omean, ovar = _np_fit_predict(xn, y, bounds, layers, (xs - mu) / sd, tb)
    assert _rel(mean, omean) < 1e-8 and _rel(var, ovar) < 1e-8


def test_single_block_composition_learns_the_same(ca, monkeypatch):
    from cimrgp_amd import Posteriors
    x, y, _ = _data(n=1001)
    idx = ca.IndexSetUniform(x.shape[0], 2, 2)
    thetas = []
    for cap in (Posteriors.BATCH_MAX_N, 64):
        monkeypatch.setattr(Posteriors, "BATCH_MAX_N", cap)
        m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=_kernels(ca, (0, 2, 0), 2),
                                              optimize_hyperparameters=True)
        m.fit()
        thetas.append(np.array([[p.kernel.sf, p.kernel.l, p.kernel.noise] for p in m.posterior_obj]))
    np.testing.assert_allclose(thetas[1], thetas[0], rtol=1e-6)


def test_layer_log_marginal_likelihood(ca):
    x, y, _ = _data(n=1001)
    n, res = x.shape[0], 2
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2),
                                          spectral_density_obj=_kernels(ca, (0, 0, 0), res), optimize_hyperparameters=True)
    m.fit()
    xn = oracle.normalize_inputs(x)[0]
    bounds = oracle.index_bounds_uniform(n, res, 2)
    layers = [(0, p.kernel.l, p.kernel.sf, p.kernel.noise) for p in m.posterior_obj]
    j = 1
    f_bar = _fbar(xn, y, bounds, layers[:j])
    for ell, sf, noise in [(0.3, 0.8, 0.02), (0.9, 1.5, 0.1)]:
        lml, grad = m.layer_log_marginal_likelihood(j, ell, sf, noise)
        want, wgrad = 0.0, np.zeros(3)
        for a, b in bounds[j]:
            r = y[a:b] - f_bar[a:b]
            v, g = np_lml_grad(xn[a:b], r - r.mean(axis=0), 0, ell, sf, noise)
            want, wgrad = want + v, wgrad + g
        assert abs(lml - want) < 1e-9 * abs(want) and _rel(grad, wgrad) < 1e-7
    k = m.posterior_obj[j].kernel
    at_opt = m.layer_log_marginal_likelihood(j, k.l, k.sf, k.noise)[0]
    at_start = m.layer_log_marginal_likelihood(j, 0.5, 1.0, 0.01)[0]
    assert at_opt >= at_start


def test_default_path_is_unchanged(ca):
    x, y, xs = _data(n=700, ns=100)
    idx, tidx = ca.IndexSetUniform(x.shape[0], 2, 2), ca.IndexSetUniform(xs.shape[0], 2, 2)
    out = []
    for kw in ({}, dict(optimize_hyperparameters=False)):
        m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=_kernels(ca, (0, 2, 0), 2), **kw)
        m.fit()
        out.append(m.get_predicted_mean_and_var(xs, tidx) + (m._f_bar_final.cpu().numpy(),))
        assert all(r is None for r in m.optimizer_results)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _two_rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    x, y, xs = _data(n=640, ns=200, seed=21)
    res = 3
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(x.shape[0], res, 2),
                                              spectral_density_obj=_kernels(ca, (0, 0, 2, 0), res), optimize_hyperparameters=True)
    model.fit()
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], res, 2))
    theta = np.array([[p.kernel.sf, p.kernel.l, p.kernel.noise] for p in model.posterior_obj])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mean=mean, var=var, theta=theta)
    td.destroy_process_group()


def test_two_ranks_learn_what_one_rank_learns(ca, tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    x, y, xs = _data(n=640, ns=200, seed=21)
    res = 3
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(x.shape[0], res, 2),
                                              spectral_density_obj=_kernels(ca, (0, 0, 2, 0), res), optimize_hyperparameters=True)
    model.fit()
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], res, 2))
    theta = np.array([[p.kernel.sf, p.kernel.l, p.kernel.noise] for p in model.posterior_obj])
    for r in range(2):
        g = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        np.testing.assert_allclose(g["theta"], theta, rtol=1e-6)
        assert _rel(g["mean"], mean) < 1e-7 and _rel(g["var"], var) < 1e-7
