"""GPU tests of the gradient of the bound on uncertain inputs above the kernels ("Gradients of the bound on
uncertain inputs"): ``UncertainInputBlock.bound_grad`` / ``elbo_grad`` against the oracle of tests/psi_grad_numpy.py, and the
``BayesianGPLVM`` plugin.

The rule is that of tests/test_gpu_psi_model.py (``psi_numpy.allowance``): every case evaluates the oracle in float64 and in
longdouble and allows a device quantity 10 x |float64 - longdouble| of that quantity off the longdouble value; a vector is one
quantity (both sides of the rule are its largest entry); the floor, 1e-10, is taken relative to the largest entry of the
whole gradient."""
import functools

import numpy as np
import pytest

import psi_grad_numpy as pg
import psi_numpy as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, NS = 300, 40
SF, NOISE, EPS = 1.3, 0.3, 1e-6
ELLS = [0.9, 1.4, 1.1]
LD = np.longdouble
#: (m, d, q, ARD, a shared variance vector, a given prior): every m, d, q and every option in both states
CASES = [(32, 1, 1, False, False, False), (32, 1, 2, True, True, True), (32, 3, 1, True, False, True), (32, 3, 2, False, True, False),
         (64, 1, 1, True, True, False), (64, 1, 2, False, False, True), (64, 3, 1, False, True, True), (64, 3, 2, True, False, False)]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", torch.float64).contiguous()


@functools.lru_cache(maxsize=None)
def _problem(m, d, q, ard, shared, prior):
    mu, s, z, y = po.problem(N, m, d, 1000 * m + 10 * d + q, q=q, far=False)
    if shared:
        s = np.array([0.3, 0.0, 2.5][:d]) if d > 1 else np.array([0.3])
    ell = np.array(ELLS[:d]) if ard else 0.9
    rng = np.random.RandomState(m + d + q)
    pm, pv = (mu + 0.1 * rng.randn(N, d), rng.uniform(0.2, 2.0, size=(N, d))) if prior else (None, None)
    refs = [pg.elbo_grad(mu, s, z, y, ell, SF, NOISE, EPS, pm, pv, ft) + (pg.kl_parts(mu, np.broadcast_to(s, (N, d)), pm, pv, ft),)
            for ft in (np.float64, LD)]
    return mu, s, z, y, ell, pm, pv, refs


def _block(ca, mu, var, z, ell, ard, pm, pv):
    from cimrgp_amd.KernelClass import RBFKernel
    kw = dict(prior_mean=None if pm is None else _dev(pm), prior_var=None if pv is None else _dev(pv))
    if ard:
        kw['lengthscales'] = ell
    return ca.UncertainInputBlock(_dev(mu), var, _dev(z), RBFKernel(l=1.0 if ard else ell, sf=SF, noise=NOISE), EPS, **kw)


def _flat(g, ard):
    """The oracle's gradient as the block returns it: dtheta with one log l unless ARD."""
    dl = np.asarray(g['dl']) if ard else np.asarray(g['dl']).sum(keepdims=True)
    return dict(dtheta=np.concatenate([[g['dsf']], dl, [g['dnoise']]]), dz=g['dz'], dmu=g['dmu'], ds=g['ds'])


def _within(got, v64, vld, floor, what):
    err = float(np.abs(np.asarray(got, dtype=LD) - vld).max())
    own = float(np.abs(np.asarray(v64, dtype=LD) - vld).max())
    allowed = max(10.0 * own, floor)
    print("%s: device - longdouble %.3e, float64 - longdouble %.3e, allowed %.3e" % (what, err, own, allowed))
    return err <= allowed


@pytest.mark.parametrize("m,d,q,ard,shared,prior", CASES)
def test_bound_grad_and_elbo_grad_match_the_oracle(ca, m, d, q, ard, shared, prior):
    mu, s, z, y, ell, pm, pv, ((e64, g64, k64), (eld, gld, kld)) = _problem(m, d, q, ard, shared, prior)
    blk = _block(ca, mu, s if shared else _dev(s), z, ell, ard, pm, pv).fit(_dev(y))
    f, dtheta, dz, dmu, ds = blk.bound_grad()
    assert f == blk.bound()                                              # the F returned is bound()'s, to the bit
    fe, dtheta_e, dz_e, dmu_e, ds_e = blk.elbo_grad()
    assert fe == f - blk.kl() and np.array_equal(dtheta, dtheta_e) and torch.equal(dz, dz_e)
    a64, ald = _flat(g64, ard), _flat(gld, ard)
    floor = 1e-10 * max(float(np.abs(v).max()) for v in ald.values())
    ok = _within(f, e64 + k64[0], eld + kld[0], 1e-10 * abs(float(eld + kld[0])), "F")
    ok &= _within(fe, e64, eld, 1e-10 * abs(float(eld)), "F - KL")
    ok &= _within(blk.kl(), k64[0], kld[0], 1e-10 * abs(float(kld[0])), "KL")
    ok &= _within(dtheta, a64['dtheta'], ald['dtheta'], floor, "dtheta")
    ok &= _within(dz.cpu().numpy(), a64['dz'], ald['dz'], floor, "dZ")
    ok &= _within(dmu_e.cpu().numpy(), a64['dmu'], ald['dmu'], floor, "dmu (F - KL)")
    ok &= _within(ds_e.cpu().numpy(), a64['ds'], ald['ds'], floor, "ds (F - KL)")
    ok &= _within(dmu.cpu().numpy(), a64['dmu'] + k64[1], ald['dmu'] + kld[1], floor, "dmu (F)")
    ok &= _within(ds.cpu().numpy(), a64['ds'] + k64[2], ald['ds'] + kld[2], floor, "ds (F)")
    assert ok
    # what is not wanted is not returned; the rest is the same
    f2, dtheta2, dz2, dmu2, ds2 = blk.bound_grad(want_z=False, want_inputs=False)
    assert f2 == f and np.array_equal(dtheta2, dtheta) and dz2 is None and dmu2 is None and ds2 is None
    with pytest.raises(TypeError, match="not yet supported"):
        blk.lml_grad(_dev(y))


# ---- the plugin ------------------------------------------------------------------------------------------------------
def _data(n, d, q, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-2.0, 3.0, size=(n, d)) * np.array([1.0, 4.0, 0.5][:d])
    y = np.sin(x @ rng.randn(d, q)) + 0.1 * rng.randn(n, q) + 2.0
    return x, y, rng.uniform(-2.0, 3.0, size=(NS, d)) * np.array([1.0, 4.0, 0.5][:d])


def test_analytic_optimize_does_not_lower_the_bound(ca):
    from cimrgp_amd.GPLVM import BayesianGPLVM
    x, y, xs = _data(300, 2, 1, 5)
    fixed = BayesianGPLVM(num_inducing=32)
    fixed.fit([x, y])
    learned = BayesianGPLVM(num_inducing=32, optimize=True, max_iters=5)
    learned.fit([x, y])
    both = BayesianGPLVM(num_inducing=32, optimize=True, max_iters=5, optimize_inducing=True)
    both.fit([x, y])
    print("bound: fixed %.6f, analytic, 5 iterations %.6f, with Z %.6f" % (fixed.block.bound(), learned.block.bound(), both.block.bound()))
    for g in (learned, both):
        assert g.optimizer_result is not None and g.optimizer_result.nit <= 5
        assert g.block.bound() >= fixed.block.bound() and g.elbo() >= fixed.elbo()
        assert g.lengthscales.shape == (2,) and np.isfinite(g.predict(xs)).all()
        # the inputs' distributions were not learned: the prior N(observed inputs, X_var) keeps KL = 0
        assert g.kl_divergence() == 0.0 and np.allclose(g.input_means, x, rtol=0, atol=1e-12)
    assert np.array_equal(learned.inducing_inputs, fixed.inducing_inputs) and not np.array_equal(both.inducing_inputs, fixed.inducing_inputs)
    f, dtheta, dz, dmu, ds = learned.elbo_grad()
    assert f == learned.elbo() and dtheta.shape == (4,) and dz.shape == (32, 2) and dmu.shape == ds.shape == (300, 2)
    # the standard prior is the parent's KL
    std = BayesianGPLVM(num_inducing=32, input_prior='standard')
    std.fit([x, y])
    parent = ca.BGPLVM(num_inducing=32)
    parent.fit([x, y])
    assert std.kl_divergence() == parent.kl_divergence() and std.elbo() == parent.elbo()


def _noisy_inputs(n, v, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-2.0, 2.0, size=(n, 1))
    y = np.hstack([np.sin(2.0 * x), np.cos(1.5 * x), np.tanh(x)]) + 0.05 * rng.randn(n, 3)
    return x, x + np.sqrt(v) * rng.randn(n, 1), y


def test_learned_inputs_move_towards_the_clean_inputs(ca):
    """Clean x, observed x + N(0, v) given with X_var = v, three outputs with noise 0.05; n = 300, v = 0.09, seed 3, 32 inducing
    inputs, noise started at 0.05, 30 L-BFGS-B iterations over [theta, mu, log s].  The data were chosen on the float64 ORACLE
    (tests/psi_grad_numpy.py ``elbo_grad`` through ``Hyper.minimize_lml`` on the CPU, the same vector and start): it takes
    F - KL from -2530.97 to 236.50 and the RMSE of the means to the clean inputs from 0.3036 (the observed inputs) to 0.0972,
    a factor 3.12 where the test asks for more than 1 -- chosen for a factor of at least 2 to spare, not tuned on the device."""
    from cimrgp_amd.GPLVM import BayesianGPLVM
    n, v = 300, 0.09
    x, xo, y = _noisy_inputs(n, v, 3)
    kw = dict(num_inducing=32, X_var=v, noise=0.05)
    before = BayesianGPLVM(**kw)
    before.fit([xo, y])
    g = BayesianGPLVM(optimize=True, max_iters=30, optimize_inputs=True, **kw)
    g.fit([xo, y])
    rmse = lambda a: float(np.sqrt(((a - x) ** 2).mean()))
    print("F - KL: before %.4f, after %.4f; rmse to the clean inputs: observed %.4f, learned %.4f" % (
        before.elbo(), g.elbo(), rmse(xo), rmse(g.input_means)))
    assert before.kl_divergence() == 0.0 and g.kl_divergence() > 0.0
    assert g.elbo() >= before.elbo()
    assert rmse(g.input_means) < rmse(xo)
    assert g.input_means.shape == (n, 1) and g.input_variances.shape == (n, 1) and (g.input_variances > 0).all()
    assert isinstance(g.block.x_var, torch.Tensor)                       # a shared X_var became per-row


def test_bgplvm_itself_is_unchanged(ca):
    """``BGPLVM`` goes through ``UncertainInputBlock.fit`` with the arguments it always passed: its elbo() and predictions are,
    to the bit, those of that block built by hand -- with and without the new (default) prior arguments."""
    from cimrgp_amd.KernelClass import RBFKernel
    x, y, xs = _data(300, 2, 2, 9)
    g = ca.BGPLVM(num_inducing=48, X_var=np.full((300, 2), 0.02))
    g.fit([x, y])
    blk = ca.UncertainInputBlock(g._x, g._var, g._z, RBFKernel(l=1.0, sf=1.0, noise=1.0), 1e-6, lengthscales=np.ones(2)).fit(g._y)
    assert g.block.prior_mean is None and g.block.prior_var is None
    assert g.elbo() == blk.elbo() and g.kl_divergence() == blk.kl()
    xt = torch.as_tensor((xs - g.data_mean) / g.data_std).to("cuda", torch.float64).contiguous()
    mean = torch.empty((NS, 2), dtype=torch.float64, device="cuda")
    var = torch.empty(NS, dtype=torch.float64, device="cuda")
    blk.predict(xt, mean, var)
    pm, pvar = g.predict_with_variance(xs)
    assert np.array_equal(pm, mean.cpu().numpy() * g.labels_std + g.labels_mean) and np.array_equal(pvar, var.cpu().numpy())
