"""ARD length-scales in the multiresolution model ("ARD length-scales for the model's layers"): a model with ARD
kernels against the isotropic model built on pre-scaled inputs (the same device calls on the same numbers), against the
NumPy chain of tests/layer_ard_numpy.py, sparse ARD layers, per-layer learning of d length-scales against a NumPy
L-BFGS-B driver, the single-block fall-back, layer_log_marginal_likelihood with a vector, and two ranks.

Inputs are 2-D; N = 1201 with divider 2 and two resolutions gives regions of 1201, 600 / 601 and 300 / 300 / 300 / 301 rows
(batched and single-block calls in one model); 301 test points with their own index set."""
import os

import numpy as np
import pytest

import layer_ard_numpy as la
import sparse_ard_numpy as sa
from grad_numpy import central_diff
from layer_ard_numpy import rel as _rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, NS, RES, DIV = 1201, 301, 2, 2
NOISE = 0.05
ELLS = np.array([0.6, 1.8])                       # l o [1, 3]: x_1 spans three times the range of x_0


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _problem(n=N, ns=NS, seed=0):
    from cimrgp_amd.Inputs import space_filling_order
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, 2)) * np.array([1.0, 3.0])
    x = x[space_filling_order(x)]
    y = np.stack([np.sin(2 * x[:, 0]) + 0.2 * x[:, 1], np.cos(1.5 * x[:, 0]) * np.cos(0.4 * x[:, 1])], axis=1)
    y = y + 0.05 * rng.normal(size=(n, 2))
    xs = rng.uniform(-1.8, 1.8, size=(ns, 2)) * np.array([1.0, 3.0])
    return x, y, xs[space_filling_order(xs)]


def _kernel(ca, cov, l, sf=1.0, noise=NOISE):
    return ca.RBFKernel(l=l, sf=sf, noise=noise) if cov == 0 else ca.DenseMaternKernel(la.COVS[cov], l=l, sf=sf, noise=noise)


def _fit(ca, x, y, kernels, res=RES, **kw):
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(x.shape[0], res, DIV),
                                          spectral_density_obj=kernels, **kw)
    m.fit()
    return m


def _close(a, b, what):
    """The project's bar for two routes through the same device calls (1e-12 relative); says whether they are bit-equal."""
    gap = _rel(a, b)
    print("%s: gap %.3e%s" % (what, gap, " (bit-equal)" if np.array_equal(a, b) else ""))
    assert np.isfinite(np.asarray(a)).all() and gap <= 1e-12, (what, gap)


# ---- 1. equivalence with pre-scaled inputs -------------------------------------------------------------------------------
@pytest.mark.parametrize("cov,res", [(0, RES), (2, RES), (0, 0)])
def test_ard_model_equals_the_isotropic_model_on_scaled_inputs(ca, cov, res):
    x, y, xs = _problem()
    scale = 1.0 / ELLS
    sfs = [1.0, 0.5, 0.25][:res + 1]
    a = _fit(ca, x, y, [_kernel(ca, cov, ELLS, sf) for sf in sfs], res, standard_normalized_inputs=False)
    b = _fit(ca, x * scale, y, [_kernel(ca, cov, 1.0, sf) for sf in sfs], res, standard_normalized_inputs=False)
    assert all(p.kernel.ard for p in a.posterior_obj) and not any(p.kernel.ard for p in b.posterior_obj)
    if res:
        assert any(len(bt.regions) >= 2 for p in a.posterior_obj for bt in p.batches)       # the batched calls are in it
    ia, ib = (ca.IndexSetUniform(NS, res, DIV), ca.IndexSetUniform(NS, res, DIV)) if res else (None, None)
    xb = xs * scale
    for got, want, what in zip(a.get_predicted_mean_and_var(xs, ia), b.get_predicted_mean_and_var(xb, ib), ("mean", "variance")):
        _close(got, want, what)
    _close(a.get_predicted_mean(xs, ia), b.get_predicted_mean(xb, ib), "mean alone")
    _close(a._f_bar_final.cpu().numpy(), b._f_bar_final.cpu().numpy(), "training-point chain")
    _close(a.get_predicted_covariance(xs, ia), b.get_predicted_covariance(xb, ib), "joint covariance")
    _close(a.posterior_samples(xs, 3, ia, seed=5), b.posterior_samples(xb, 3, ib, seed=5), "samples")
    for got, want, what in zip(a.leave_one_out(), b.leave_one_out(), ("leave-one-out mean", "leave-one-out variance")):
        _close(got, want, what)
    (am, av), (bm, bv) = a.predictive_gradients(xs, ia), b.predictive_gradients(xb, ib)
    assert am.shape == (NS, 2, 2) and av.shape == (NS, 2)
    _close(am, bm * scale[None, :, None], "gradient of the mean")
    _close(av, bv * scale[None, :], "gradient of the variance")


def test_fp32_model_takes_ard(ca):
    x, y, xs = _problem()
    ks = [_kernel(ca, 0, ELLS, sf, noise=0.1) for sf in (1.0, 0.5, 0.25)]
    m32 = _fit(ca, x, y, ks, dtype='f32', standard_normalized_inputs=False)
    m64 = _fit(ca, x, y, ks, standard_normalized_inputs=False)
    idx = ca.IndexSetUniform(NS, RES, DIV)
    mean32, var32 = m32.get_predicted_mean_and_var(xs, idx)
    mean64, var64 = m64.get_predicted_mean_and_var(xs, idx)
    assert _rel(mean32, mean64) < 1e-3 and _rel(var32, var64) < 1e-3       # the FP32 bar of the layer objective's test


# ---- 2. against NumPy -------------------------------------------------------------------------------------------------------
MIXES = {   # ARD and isotropic layers mixed: [(cov, l)]
    "rbf": [(0, np.array([0.9, 0.5])), (0, 0.5), (0, np.array([0.4, 0.2]))],
    "mixed": [(2, np.array([0.9, 0.5])), (0, 0.5), (3, np.array([0.4, 0.2]))],
}


@pytest.mark.parametrize("which", sorted(MIXES))
def test_mixed_model_matches_the_numpy_chain_and_central_differences(ca, which):
    import oracle
    x, y, xs = _problem()
    sfs = (1.0, 0.5, 0.25)
    kernels = [_kernel(ca, cov, l, sf) for (cov, l), sf in zip(MIXES[which], sfs)]
    m = _fit(ca, x, y, kernels)                                      # standard_normalized_inputs=True, the default
    assert [p.kernel.ard for p in m.posterior_obj] == [True, False, True]
    idx = ca.IndexSetUniform(NS, RES, DIV)
    mean, var = m.get_predicted_mean_and_var(xs, idx)
    xn, _, mu, sd = oracle.normalize_inputs(x)
    layers = [(cov, l, sf, NOISE) for (cov, l), sf in zip(MIXES[which], sfs)]
    _, _, wmean, wvar = la.fit_predict(xn, y, oracle.index_bounds_uniform(N, RES, DIV), layers, (xs - mu) / sd,
                                       oracle.index_bounds_uniform(NS, RES, DIV))
    print("%s: mean gap %.3e, variance gap %.3e" % (which, _rel(mean, wmean), _rel(var, wvar)))
    assert _rel(mean, wmean) < 1e-8 and _rel(var, wvar) < 1e-8
    # step and bars of tests/test_gpu_grad.py's central-difference test, in the caller's units
    dmu, dvar = m.predictive_gradients(xs, idx)
    fm, fv = central_diff(lambda t: m.get_predicted_mean_and_var(t, idx), xs, 1e-5 * np.abs(xs).max())
    tol = 1e-6 if which == "rbf" else 2e-5
    print("%s: gradient gaps %.3e %.3e (bar %.0e)" % (which, _rel(dmu, fm), _rel(dvar, fv), tol))
    assert _rel(dmu, fm) < tol and _rel(dvar, fv) < tol


# ---- 3. sparse ARD layers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("approximation", ["fitc", "vfe"])
def test_sparse_ard_layers_equal_the_isotropic_model_on_scaled_inputs(ca, approximation):
    x, y, xs = _problem()
    scale = 1.0 / ELLS

    def kernels(l):
        sparse = [ca.SparseKernel(_kernel(ca, 0, l, sf), num_inducing=130, approximation=approximation) for sf in (1.0, 0.5)]
        return sparse + [_kernel(ca, 0, l, 0.25)]

    a = _fit(ca, x, y, kernels(ELLS), standard_normalized_inputs=False)
    b = _fit(ca, x * scale, y, kernels(1.0), standard_normalized_inputs=False)
    assert all(p.kernel.ard for p in a.posterior_obj)
    idx = ca.IndexSetUniform(NS, RES, DIV)
    for noise in (True, False):
        got = a.get_predicted_mean_and_var(xs, idx, include_noise=noise)
        want = b.get_predicted_mean_and_var(xs * scale, idx, include_noise=noise)
        _close(got[0], want[0], "mean")
        _close(got[1], want[1], "variance (noise %s)" % noise)
    _close(a.get_predicted_mean(xs, idx), b.get_predicted_mean(xs * scale, idx), "mean alone")
    _close(a._f_bar_final.cpu().numpy(), b._f_bar_final.cpu().numpy(), "training-point chain")
    for call in (lambda: a.predictive_gradients(xs, idx), lambda: a.get_predicted_covariance(xs, idx),
                 lambda: a.posterior_samples(xs, 2, idx), lambda: a.leave_one_out(0), lambda: a.leave_one_out(1)):
        with pytest.raises(TypeError, match="not yet supported"):
            call()
    mean, var = a.leave_one_out(2)                                   # the exact ARD layer keeps its leave-one-out
    assert mean.shape == (N, 2) and np.isfinite(var).all()


# ---- 4. learning ----------------------------------------------------------------------------------------------------------
def learn_problem(n=N, ns=NS, seed=3):
    """Clearly anisotropic, at three scales: every component of the four targets varies about three times faster along
    x_0 than along x_1 (both z-scored by the model).  With LEARN_STARTS each layer has an inexact (inducing-point) layer
    above it, so that the slow structure is the root's, the middle one layer 1's and the fast one is left to the exact
    ARD layer 2: every learned layer has an interior optimum.  Checked on the CPU with the NumPy driver alone, from the
    starts x 1 and x 1.001: all 11 learned values agree to 1.5e-6 or better at N = 1201 (root l = [1.30, 3.20], layer 1
    l = 0.99, layer 2 l = [0.100, 0.268], sf = 3.2 / 0.17 / 0.021, noise = 0.049 / 0.015 / 0.00088).  The smaller sets of the fall-back test (n = 1001, seed 3) and
    of the two-rank test (n = 640, seed 21) have interior optima too (layer 2: sf = 0.019 / 0.016, l = [0.095, 0.263] /
    [0.091, 0.251]); there the two starts agree to 7e-6 or better in the two sparse layers and to 1.1e-4 / 2.1e-5 at worst
    (the noise of layer 2) in the exact one.  Those two tests compare two routes from the SAME start."""
    from cimrgp_amd.Inputs import space_filling_order
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, 2))
    x = x[space_filling_order(x)]
    cols = [np.sin(1.5 * x[:, 0] + c) * np.cos(0.5 * x[:, 1]) + 0.3 * np.sin(5 * x[:, 0] + 1.7 * x[:, 1] + c)
            + 0.12 * np.sin(14 * x[:, 0] + 4.5 * x[:, 1] + 2 * c) for c in range(4)]
    y = np.stack(cols, axis=1) + 0.03 * rng.normal(size=(n, 4))
    xs = rng.uniform(-1.8, 1.8, size=(ns, 2))
    return x, y, xs[space_filling_order(xs)]


#: the constructor's kernels of the learning tests, (cov, l, sparse) per layer: ARD started at [1, 1] 2^-j -- a FITC root
#: of 16 inducing inputs and the exact layer 2, whose four regions go through the batched ARD objective -- and one isotropic
#: layer, VFE with 48 inducing inputs
LEARN_STARTS = [(0, np.array([1.0, 1.0]), la.Sparse(16, 0)), (2, 0.5, la.Sparse(48, 1)), (0, np.array([0.25, 0.25]), None)]


def _learn_kernels(ca, starts=LEARN_STARTS):
    ks = []
    for cov, l, sp in starts:
        k = _kernel(ca, cov, l, 1.0, noise=None)
        ks.append(k if sp is None else ca.SparseKernel(k, num_inducing=sp.m, approximation=('fitc', 'vfe')[sp.mode], jitter=sp.eps))
    return ks


def _driver_starts(starts=LEARN_STARTS):
    return [(cov, l, 1.0) + (() if sp is None else (sp,)) for cov, l, sp in starts]


def _theta(model):
    return np.concatenate([np.concatenate([[p.kernel.sf], np.atleast_1d(p.kernel.l), [p.kernel.noise]]) for p in model.posterior_obj])


def test_model_learns_what_the_numpy_driver_learns(ca):
    import oracle
    x, y, xs = learn_problem()
    kernels = _learn_kernels(ca)
    model = _fit(ca, x, y, kernels, optimize_hyperparameters=True)
    idx = ca.IndexSetUniform(NS, RES, DIV)
    mean, var = model.get_predicted_mean_and_var(xs, idx)
    xn, _, mu, sd = oracle.normalize_inputs(x)
    bounds = oracle.index_bounds_uniform(N, RES, DIV)
    layers, results = la.learn(xn, y, bounds, _driver_starts())
    assert layers[0][1][1] > layers[0][1][0]                         # the driver finds the anisotropy
    for j, (cov, l0, _) in enumerate(LEARN_STARTS):
        k = model.posterior_obj[j].kernel
        assert k is not kernels[j] and type(k) is type(kernels[j])
        assert kernels[j].noise is None and np.array_equal(kernels[j].l, l0)         # the caller's objects are untouched
        ell, sf2, noise = layers[j][1:4]
        if np.ndim(l0):
            assert k.ard is True and k.l.shape == (2,)
        else:
            assert k.ard is False and type(k.l) is float
        print("layer %d: l %s sf %.6g noise %.6g; driver l %s" % (j, k.l, k.sf, k.noise, ell))
        np.testing.assert_allclose(np.concatenate([[k.sf], np.atleast_1d(k.l), [k.noise]]),
                                   np.concatenate([[sf2], np.atleast_1d(ell), [noise]]), rtol=1e-5)
        assert abs(model.optimizer_results[j].fun - results[j].fun) < 1e-8 * abs(results[j].fun)
    _, _, wmean, wvar = la.fit_predict(xn, y, bounds, layers, (xs - mu) / sd, oracle.index_bounds_uniform(NS, RES, DIV))
    assert _rel(mean, wmean) < 1e-8 and _rel(var, wvar) < 1e-8


# ---- 5. single-block fall-back --------------------------------------------------------------------------------------------
def test_single_block_composition_learns_the_same(ca, monkeypatch):
    from cimrgp_amd import Posteriors
    x, y, _ = learn_problem(n=1001)
    thetas = []
    for cap in (Posteriors.BATCH_MAX_N, 64):
        monkeypatch.setattr(Posteriors, "BATCH_MAX_N", cap)
        thetas.append(_theta(_fit(ca, x, y, _learn_kernels(ca), optimize_hyperparameters=True)))
    np.testing.assert_allclose(thetas[1], thetas[0], rtol=1e-6)


# ---- 6. layer_log_marginal_likelihood ---------------------------------------------------------------------------------------
POINTS = [(np.array([0.3, 0.8]), 0.8, 0.02), (np.array([0.9, 0.4]), 1.5, 0.1)]


def test_layer_log_marginal_likelihood_of_a_dense_layer_takes_a_vector(ca):
    import oracle
    x, y, _ = _problem()
    specs = [(0, np.array([0.9, 0.5])), (2, 0.5), (0, 0.3)]          # layer 1, asked below, is isotropic itself
    m = _fit(ca, x, y, [_kernel(ca, cov, l) for cov, l in specs])
    xn = oracle.normalize_inputs(x)[0]
    bounds = oracle.index_bounds_uniform(N, RES, DIV)
    before = la.fit_predict(xn, y, bounds, [(cov, l, 1.0, NOISE) for cov, l in specs])[1]
    for j in (0, 1, 2):
        for ell, sf, noise in POINTS:
            lml, grad = m.layer_log_marginal_likelihood(j, ell, sf, noise)
            want, wgrad = la.layer_objective(xn, y - before[j], bounds[j], specs[j][0], ell, sf, noise)
            assert grad.shape == (4,)
            assert abs(lml - want) < 1e-9 * abs(want) and _rel(grad, wgrad) < 1e-7, (j, _rel(grad, wgrad))
    lml, grad = m.layer_log_marginal_likelihood(0, 0.7, 0.8, 0.02)   # a scalar on an ARD layer: the isotropic objective
    want, wgrad = la.layer_objective(xn, y, bounds[0], 0, 0.7, 0.8, 0.02)
    assert grad.shape == (3,) and abs(lml - want) < 1e-9 * abs(want) and _rel(grad, wgrad) < 1e-7


@pytest.mark.parametrize("mode", [0, 1])
def test_layer_log_marginal_likelihood_of_a_sparse_layer_takes_a_vector(ca, mode):
    """Against the sum over the regions of the NumPy chain form, at 100 x the gap between that form and the autograd of the
    restated chain (relative, floor 1e-9): the bar of tests/test_gpu_sparse_layer.py."""
    import oracle
    x, y, _ = _problem()
    cov, eps = 2, 1e-6
    sk = ca.SparseKernel(_kernel(ca, cov, np.array([0.9, 0.5])), num_inducing=130, approximation=('fitc', 'vfe')[mode], jitter=eps)
    m = _fit(ca, x, y, [sk, _kernel(ca, 0, 0.5), _kernel(ca, 0, np.array([0.4, 0.2]))])
    xn = oracle.normalize_inputs(x)[0]
    z = xn[sk.inducing_rows(0, 0, N)]
    r = y - y.mean(axis=0)
    for ell, sf, noise in POINTS:
        lc, gc, _ = sa.chain(xn, z, r, cov, ell, sf, noise, eps, mode)
        lauto, gauto, _ = sa.autograd(xn, z, r, cov, ell, sf, noise, eps, mode, want_z=False)
        tol_l, tol_g = max(1e-9, 100 * _rel(lauto, lc)), max(1e-9, 100 * _rel(gauto, gc))
        lml, grad = m.layer_log_marginal_likelihood(0, ell, sf, noise)
        print("mode %d: lml gap %.3e (tolerance %.3e), grad gap %.3e (tolerance %.3e)" % (mode, _rel(lml, lc), tol_l, _rel(grad, gc), tol_g))
        assert grad.shape == (4,) and _rel(lml, lc) <= tol_l and _rel(grad, gc) <= tol_g


# ---- 7. two ranks ---------------------------------------------------------------------------------------------------------
def _two_rank_case(ca):
    x, y, xs = learn_problem(n=640, ns=200, seed=21)
    model = _fit(ca, x, y, _learn_kernels(ca), optimize_hyperparameters=True)
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], RES, DIV))
    return mean, var, _theta(model)


def _two_rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    mean, var, theta = _two_rank_case(ca)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), mean=mean, var=var, theta=theta)
    td.destroy_process_group()


def test_two_ranks_learn_what_one_rank_learns(ca, tmp_path):
    """The widened all-reduce buffer [lml | grad (d + 2) | failure] of the layer objective, in the manner of
    tests/test_gpu_layer_lml.py: two child processes on one device."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    mean, var, theta = _two_rank_case(ca)
    for r in range(2):
        g = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        np.testing.assert_allclose(g["theta"], theta, rtol=1e-6)
        assert _rel(g["mean"], mean) < 1e-7 and _rel(g["var"], var) < 1e-7
