"""GPU tests of the sparse (inducing-point) layers of MultiResolutionGaussianProcess against the NumPy chain of
tests/sparse_layer_numpy.py.  Tolerance: the project's rule (tests/test_gpu_sparse.py) -- the GPU is held to 100 x the largest
gap between the two NumPy forms (Woodbury chain, dense definition) on the same inputs, floor 1e-9; the gap is computed here,
never taken from the code under test.  Shapes: sparse_layer_numpy (N = 2801, divider 2, two resolutions, m = 130, q = 2, 701
test points)."""
import os
import socket

import numpy as np
import pytest

import sparse_layer_numpy as sl
import sparse_numpy as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NU = {1: 0.5, 2: 1.5, 3: 2.5}
MODE = {0: 'fitc', 1: 'vfe'}


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _kernels(ca, cov, mode, sparse=(0, 1), inducing='stride', m=sl.M, eps=1e-6, noise=None):
    """The kernel objects of sparse_layer_numpy.case_layers."""
    out = []
    for j in range(sl.RES + 1):
        base = ca.RBFKernel(l=sl.ELLS[j], sf=1.0, noise=noise) if cov == 0 else \
            ca.DenseMaternKernel(nu=NU[cov], l=sl.ELLS[j], sf=1.0, noise=noise)
        out.append(ca.SparseKernel(base, num_inducing=m, approximation=MODE[mode], jitter=eps, inducing=inducing, seed=3)
                   if j in sparse else base)
    return out


_MODELS = {}


def _model(ca, d, cov, mode, sparse=(0, 1), inducing='stride', m=sl.M, eps=1e-6, seed=0, **kw):
    """A fitted model of one case (fitted once per process; the tests only predict from it)."""
    key = (d, cov, mode, tuple(sparse), inducing, m, eps, seed, tuple(sorted(kw.items())))
    if key not in _MODELS:
        x, y, _, _ = sl.problem(sl.N, d, sl.NS, seed)
        model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                                  spectral_density_obj=_kernels(ca, cov, mode, sparse, inducing, m, eps), **kw)
        model.fit()
        _MODELS[key] = model
    return _MODELS[key]


def _test_set(ca, d, seed=0):
    return sl.problem(sl.N, d, sl.NS, seed)[2], ca.IndexSetUniform(sl.NS, sl.RES, sl.DIVIDER)


def _finest_noise(chain):
    """The noise the finest layer adds to each test row."""
    out = np.zeros(sl.NS)
    for blk, (a, b) in zip(chain['blocks'][-1], sl.index_bounds(sl.NS)[-1]):
        out[a:b] = blk['noise']
    return out


def _check_parity(ca, d, cov, mode, what, **case):
    """Prediction (with and without noise, mean alone) and the training-point chain of one case against the Woodbury chain,
    at 100 x the gap between the two NumPy forms (floor 1e-9)."""
    w = sl.case_chain(d, cov, mode, include_noise=False, **case)
    tol = sl.tolerance(w, sl.case_chain(d, cov, mode, form='dense', include_noise=False, **case))
    model = _model(ca, d, cov, mode, **case)
    xs, idx = _test_set(ca, d)
    mean, var = model.get_predicted_mean_and_var(xs, idx, include_noise=False)
    mean_n, var_n = model.get_predicted_mean_and_var(xs, idx)
    mean_only = model.get_predicted_mean(xs, idx)
    f_bar = model._f_bar_final.double().cpu().numpy()
    gaps = (float(np.abs(mean - w['mean']).max()), float(np.abs(var - w['var']).max()), float(np.abs(f_bar - w['f_bar']).max()),
            float(np.abs(var_n - (w['var'] + _finest_noise(w))).max()), float(np.abs(mean_only - w['mean']).max()))
    print("%s: gap mean %.3e var %.3e f_bar %.3e var+noise %.3e mean alone %.3e   tolerance mean %.3e var %.3e f_bar %.3e"
          % ((what,) + gaps + tol))
    assert np.isfinite(mean).all() and np.isfinite(var).all() and (var > 0).all()
    assert gaps[0] <= tol[0] and gaps[1] <= tol[1] and gaps[2] <= tol[2] and gaps[3] <= tol[1] and gaps[4] <= tol[0]
    assert np.array_equal(mean_n, mean)          # (the mean alone takes the fused product in the exact layers: not bit-equal)
    return model, w


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("d", [1, 2])
def test_sparse_layers_match_the_numpy_chain(ca, d, cov, mode):
    """Layers 0 and 1 sparse (m = 130), layer 2 exact: prediction and the chain at the training points."""
    model, w = _check_parity(ca, d, cov, mode, "d=%d cov=%d %s" % (d, cov, MODE[mode]))
    assert [type(p).__name__ for p in model.posterior_obj] == ['SparsePosterior', 'SparsePosterior', 'DensePosterior']
    for j in (0, 1):
        for l, blk in enumerate(w['blocks'][j]):
            assert np.array_equal(model.posterior_obj[j].inducing_rows(l), blk['rows'])
            assert model.posterior_obj[j].blocks[l].m == sl.M


def test_all_layers_sparse_with_random_inducing_rows(ca):
    model, w = _check_parity(ca, 2, 0, 0, "all sparse, random rows", sparse=(0, 1, 2), inducing='random')
    xs, idx = _test_set(ca, 2)
    # the mean alone takes the sparse blocks' own route (W* gamma): the same numbers
    assert np.array_equal(model.get_predicted_mean(xs, idx), model.get_predicted_mean_and_var(xs, idx)[0])
    for j in range(3):
        for l, blk in enumerate(w['blocks'][j]):
            n_l = model.n_samps[j][l]
            assert np.array_equal(model.posterior_obj[j].inducing_rows(l), np.random.RandomState([3, j, l]).permutation(n_l)[:sl.M])
            assert np.array_equal(model.posterior_obj[j].inducing_rows(l), blk['rows'])


@pytest.mark.parametrize("flag", ["noise_region_specific", "bias_region_specific"])
def test_shared_noise_and_shared_bias(ca, flag):
    _check_parity(ca, 1, 0, 0, flag + "=False", **{flag: False})


@pytest.mark.parametrize("d", [1, 2])
def test_inducing_at_the_data_gives_the_all_exact_model(ca, d):
    """num_inducing >= n, jitter 0, Matern 1/2: Z = X in every sparse block, so the model is the all-exact one -- bias, noise
    rule, chain and variance sum against the existing path.  Tolerance: 100 x the gap between the NumPy Z = X chain and
    the NumPy exact chain (floor 1e-9)."""
    s_np = sl.case_chain(d, 1, 0, sparse=(0, 1), m=4000, eps=0.0, include_noise=False)
    e_np = sl.case_chain(d, 1, 0, sparse=(), include_noise=False)
    tol = sl.tolerance(s_np, e_np)
    sparse = _model(ca, d, 1, 0, sparse=(0, 1), m=4000, eps=0.0)
    exact = _model(ca, d, 1, 0, sparse=())
    assert sparse.posterior_obj[0].blocks[0].m == sl.N and sparse.posterior_obj[1].blocks[1].m == 1401
    xs, idx = _test_set(ca, d)
    for noise in (False, True):
        ms, vs = sparse.get_predicted_mean_and_var(xs, idx, include_noise=noise)
        me, ve = exact.get_predicted_mean_and_var(xs, idx, include_noise=noise)
        gm, gv = float(np.abs(ms - me).max()), float(np.abs(vs - ve).max())
        print("Z = X d=%d noise %s: gap mean %.3e var %.3e   tolerance %.3e %.3e" % (d, noise, gm, gv, tol[0], tol[1]))
        assert gm <= tol[0] and gv <= tol[1]
    gf = float((sparse._f_bar_final - exact._f_bar_final).abs().max())
    print("Z = X d=%d: gap f_bar %.3e tolerance %.3e" % (d, gf, tol[2]))
    assert gf <= tol[2]


def test_noise_rule_of_every_block(ca):
    """kernel.noise None: each block's noise is max(0.01 var(r), 1e-8 sf) of its own residual targets (pooled population
    variance about the column means), taken here from the model's own latent function of each layer."""
    model = _model(ca, 2, 0, 0)
    _, y, _, _ = sl.problem(sl.N, 2, sl.NS, 0)
    for j, post in enumerate(model.posterior_obj):
        resid = y - model._f_bar_layers[j].double().cpu().numpy()
        for l, (a, b) in enumerate(sl.index_bounds(sl.N)[j]):
            r = resid[a:b]
            want = max(0.01 * float(np.mean((r - r.mean(axis=0)) ** 2)), 1e-8 * 1.0)
            got = float(post.blocks[l].noise.item())
            assert abs(got - want) <= 1e-12 * want, (j, l, got, want)
            assert np.abs(post.blocks[l].bias.cpu().numpy() - r.mean(axis=0)).max() <= 1e-12
    assert np.allclose(1.0 / np.array(model.stats_obj[0].noise_mean), float(model.posterior_obj[0].blocks[0].noise.item()))


def test_single_sparse_root_predicts_without_an_index_set(ca):
    x, y, xs, ys = sl.problem(sl.N, 2, sl.NS, 5)
    k = ca.SparseKernel(ca.DenseMaternKernel(nu=1.5, l=0.5), num_inducing=sl.M)
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, 0, 2), spectral_density_obj=k)
    model.fit()
    ll = model.get_test_likelihood([xs, ys])
    xn, xsn = sl.normalise(x, xs)
    w = sl.chain(xn, y, [[(0, sl.N)]], [sl.Layer(2, 0.5, m=sl.M)], xsn, [[(0, sl.NS)]], include_noise=False)
    want = np.mean(-0.5 * np.log(2 * np.pi * w['var']) - 0.5 * (np.linalg.norm(ys - w['mean'], axis=1) ** 2) / w['var'])
    print("test likelihood %.12g, NumPy %.12g" % (ll, want))
    assert np.isfinite(ll) and abs(ll - want) <= 1e-8 * abs(want)
    assert np.array_equal(model.get_predicted_mean(xs), model.get_predicted_mean_and_var(xs)[0])
    assert np.array_equal(model.get_central_moment2(xs), model.get_predicted_mean_and_var(xs)[1])


# ---- failure ----------------------------------------------------------------------------------------------------------------
def _failing_model(ca, **kw):
    """Every input row twice; layer 1 is sparse with Z = X (num_inducing >= n) and no jitter: K_uu is singular, an RBF Gram
    matrix of repeated, dense points has no positive pivots to the end.  A numerical status, not a device fault."""
    x, y, _, _ = sl.problem(sl.N, 1, sl.NS, 2, repeat=True)
    kernels = _kernels(ca, 0, 0, sparse=(0,))
    kernels[1] = ca.SparseKernel(ca.RBFKernel(l=sl.ELLS[1]), num_inducing=1500, jitter=0.0)
    return ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                             spectral_density_obj=kernels, **kw)


def test_singular_inducing_covariance_raises_and_names_the_layer(ca):
    model = _failing_model(ca)
    with pytest.raises(np.linalg.LinAlgError, match="layer 1") as e:
        model.fit()
    print(e.value)
    assert "K_uu" in str(e.value) and "not positive definite" in str(e.value)
    assert model._fitted is False
    with pytest.raises(RuntimeError, match="fit"):
        model.get_predicted_mean(np.zeros((4, 1)))


# ---- two ranks on one GPU ---------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    ca.dist.share_one_gpu()
    model = _model(ca, 2, 2, 0)
    xs, idx = _test_set(ca, 2)
    out = dict(owner1=np.asarray(model.owner[1]))
    out["mean"], out["var"] = model.get_predicted_mean_and_var(xs, idx)
    out["mean_only"] = model.get_predicted_mean(xs, idx)
    out["f_bar"] = model._f_bar_final.double().cpu().numpy()
    out["f_bar_sparse"] = model._f_bar_layers[2].double().cpu().numpy()
    for j in (0, 1):
        for l in range(model.n_regions[j]):
            out["rows%d_%d" % (j, l)] = model.posterior_obj[j].inducing_rows(l)
    bad = _failing_model(ca)
    try:
        bad.fit()
        out["raised"] = np.array("nothing")
    except np.linalg.LinAlgError as e:
        out["raised"] = np.array(str(e))
    out["bad_fitted"] = np.array(bad._fitted)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    td.barrier()
    td.destroy_process_group()


def test_two_ranks_equal_one_bit_for_bit_and_fail_together(ca, tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    model = _model(ca, 2, 2, 0)
    xs, idx = _test_set(ca, 2)
    mean, var = model.get_predicted_mean_and_var(xs, idx)
    mean_only = model.get_predicted_mean(xs, idx)
    f_bar = model._f_bar_final.double().cpu().numpy()
    f_bar_sparse = model._f_bar_layers[2].double().cpu().numpy()
    assert got[0]["owner1"].tolist() == [0, 1]                       # both ranks own sparse blocks
    for g in got:
        assert np.array_equal(g["mean"], mean) and np.array_equal(g["var"], var)
        # the mean alone reads the EXACT layer's alpha, which a rank with two equal blocks takes from the batched backward
        # solve and a rank with one from the single one (as before this model had sparse layers): 1e-12, the bar of the
        # other two-rank tests, not bit for bit
        assert _rel(g["mean_only"], mean_only) <= 1e-12
        # the chain through the two sparse layers (what layer 2 is fitted against) bit for bit; with the exact layer 1e-12
        assert np.array_equal(g["f_bar_sparse"], f_bar_sparse) and _rel(g["f_bar"], f_bar) <= 1e-12
        for j in (0, 1):
            for l in range(model.n_regions[j]):
                assert np.array_equal(g["rows%d_%d" % (j, l)], model.posterior_obj[j].inducing_rows(l))
        print(g["raised"])
        assert "layer 1" in str(g["raised"]) and "not positive definite" in str(g["raised"]) and not bool(g["bad_fitted"])


# ---- hyper-parameters -------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("j", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_layer_objective_of_a_sparse_layer(ca, j, mode):
    """Value and gradient of layer j's objective at another point of (ell, sf, noise) against the sum over its regions of
    the NumPy chain form, at 100 x the gap between that form and the autograd of the restated chain (relative, floor
    1e-9)."""
    d, cov = 2, 2
    model = _model(ca, d, cov, mode)
    x, y, xs, _ = sl.problem(sl.N, d, sl.NS, 0)
    xn, _ = sl.normalise(x, xs)
    ell, sf, noise = 0.7 * sl.ELLS[j], 1.3, 0.02
    w = sl.case_chain(d, cov, mode, include_noise=False)
    (lc, gc), (la, ga) = sl.layer_objective(xn, y - w['f_bar_layers'][j], sl.index_bounds(sl.N)[j],
                                            sl.case_layers(cov, mode)[j], j, ell, sf, noise)
    tol_l, tol_g = max(1e-9, 100 * _rel(la, lc)), max(1e-9, 100 * _rel(ga, gc))
    lml, grad = model.layer_log_marginal_likelihood(j, ell, sf, noise)
    print("layer %d %s: lml %.10g gap %.3e (tolerance %.3e), grad gap %.3e (tolerance %.3e)"
          % (j, MODE[mode], lml, _rel(lml, lc), tol_l, _rel(grad, gc), tol_g))
    assert _rel(lml, lc) <= tol_l and _rel(grad, gc) <= tol_g


def test_learning_does_not_lower_the_objective_and_rewraps_the_kernel(ca):
    d, cov, mode = 1, 0, 0
    x, y, xs, _ = sl.problem(sl.N, d, sl.NS, 0)
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                              spectral_density_obj=_kernels(ca, cov, mode), optimize_hyperparameters=True,
                                              max_iters=5)
    model.fit()
    xn, _ = sl.normalise(x, xs)
    lay = sl.case_layers(cov, mode)[0]
    z = xn[sl.inducing_rows(lay, 0, 0, sl.N)]
    rc = y - y.mean(axis=0)
    k = model.posterior_obj[0].kernel
    start = sn.woodbury(xn, z, rc, cov, sl.ELLS[0], 1.0, 0.01, lay.eps, mode)[0]
    end = sn.woodbury(xn, z, rc, cov, k.l, k.sf, k.noise, lay.eps, mode)[0]
    print("layer 0: %.6f -> %.6f at l %.4f sf %.4f noise %.5f" % (start, end, k.l, k.sf, k.noise))
    assert end >= start
    sf, ell, noise = np.exp(model.optimizer_results[0].x)
    assert isinstance(k, ca.SparseKernel) and isinstance(k.kernel, ca.RBFKernel)
    assert (k.sf, k.l, k.noise) == (float(sf), float(ell), float(noise))
    assert (k.num_inducing, k.approximation, k.jitter, k.inducing, k.seed) == (sl.M, 'fitc', 1e-6, 'stride', 3)
    assert isinstance(model.posterior_obj[1].kernel, ca.SparseKernel) and isinstance(model.posterior_obj[2].kernel, ca.RBFKernel)
    assert model.spectral_density_obj[0].l == sl.ELLS[0]            # the constructor's kernels are left as they were
    mean = model.get_predicted_mean(*_test_set(ca, d))
    assert np.isfinite(mean).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_what_sparse_layers_do_not_give_yet_is_refused(ca):
    model = _model(ca, 1, 0, 0)
    xs, idx = _test_set(ca, 1)
    for call in (lambda: model.predictive_gradients(xs, idx), lambda: model.get_predicted_covariance(xs, idx),
                 lambda: model.posterior_samples(xs, 2, idx), lambda: model.predictive_gradients(xs),
                 lambda: model.leave_one_out(0), lambda: model.get_loo_likelihood(1), lambda: model.leave_one_out(1)):
        with pytest.raises(TypeError, match="not yet supported"):
            call()
    mean, var = model.leave_one_out(2)                               # the exact layer keeps its leave-one-out
    assert mean.shape == (sl.N, 2) and np.isfinite(var).all()
    x, y, _, _ = sl.problem(sl.N, 1, sl.NS, 0)
    with pytest.raises(TypeError, match="not yet supported"):
        ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                          spectral_density_obj=_kernels(ca, 0, 0), dtype='f32')
    with pytest.raises(TypeError):
        ca.SparseKernel(ca.MaternKernel())


# ---- what was there before is unchanged -------------------------------------------------------------------------------------
def test_an_all_exact_model_is_bit_identical_beside_sparse_models(ca):
    x, y, _, _ = sl.problem(sl.N, 2, sl.NS, 0)
    xs, idx = _test_set(ca, 2)

    def exact():
        m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                              spectral_density_obj=_kernels(ca, 2, 0, sparse=()))
        m.fit()
        return m.get_predicted_mean_and_var(xs, idx) + (m.get_predicted_mean(xs, idx),)

    before = exact()
    s = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(sl.N, sl.RES, sl.DIVIDER),
                                          spectral_density_obj=_kernels(ca, 2, 1, sparse=(0, 1, 2)))
    s.fit()
    s.get_predicted_mean_and_var(xs, idx)
    after = exact()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("mode", [0, 1])
def test_sparse_block_fit_and_predict_equal_the_old_calls_by_hand(ca, mode):
    """SparseBlock.fit / predict against the calls they were made of before the layer form was added, bit for bit."""
    dev = ca.device
    n, m, d, q = 1403, 130, 2, 2
    x, z, r, xs = sn.problem(n, m, d, seed=11)
    ns = int(xs.shape[0])
    xd, zd, rd, xsd = (dev.to_device(a, torch.float64, "cuda") for a in (x, z, r, xs))
    k = ca.DenseMaternKernel(nu=1.5, l=0.6, sf=1.2, noise=0.03)
    blk = ca.SparseBlock(xd, zd, k, MODE[mode], 1e-6).fit(rd)
    mean = torch.empty((ns, q), dtype=torch.float64, device="cuda")
    var = torch.empty(ns, dtype=torch.float64, device="cuda")
    blk.predict(xsd, mean, var, include_noise=True)
    # by hand
    lu = dev.rbf_gram(zd, k.l, k.sf, 1e-6 * k.sf, lower_only=True, cov=k.cov)
    ws_u, info_u = dev.potrf(lu, m)
    a = dev.rbf_cross(xd, zd, k.l, k.sf, cov=k.cov)
    dev.trsm_rows(lu, m, ws_u, a, n)
    _, w, sums = dev.sparse_lambda(a, n, m, k.sf, k.noise, mode)
    lb, c = dev.wsyrk_tn(a, n, m, w, rd, diag_add=1.0)
    ws_b, info_b = dev.potrf(lb, m)
    gamma = dev.potrs(lb, m, ws_b, c, want_z=True)
    astar = dev.rbf_cross(xsd, zd, k.l, k.sf, cov=k.cov)
    dev.trsm_rows(lu, m, ws_u, astar, ns)
    wstar = astar.clone()
    dev.trsm_rows(lb, m, ws_b, wstar, ns)
    mean2, var2 = torch.empty_like(mean), torch.empty_like(var)
    dev.sparse_tail(astar, wstar, ns, m, gamma, k.sf, k.noise, mean2, var2)
    torch.cuda.synchronize()
    assert int(info_u.item()) == 0 and int(info_b.item()) == 0
    assert torch.equal(blk.gamma, gamma) and torch.equal(mean, mean2) and torch.equal(var, var2)
    lml = blk.log_marginal_likelihood()
    want = sn.woodbury(x, z, r, k.cov, k.l, k.sf, k.noise, 1e-6, mode)[0]
    assert abs(lml - want) <= 1e-8 * abs(want)
