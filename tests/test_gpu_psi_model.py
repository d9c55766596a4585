"""GPU tests of sparse GP regression on uncertain inputs above the kernels ("Sparse GP regression on uncertain
inputs"): ``UncertainInputBlock`` and the ``BGPLVM`` plugin against the oracle of tests/psi_numpy.py.

The two-sided solve of Psi2 by an ill-conditioned K_uu limits what float64 can do: at jitter 1e-6 the float64 oracle sits
1e-6 .. 8e-6 from its own longdouble value on F ~ 1e2 .. 1e3.  So no constant is fixed: every case evaluates the oracle in
both precisions and allows a device value 10 x |float64 - longdouble| of that quantity off the longdouble value (the factor
covers the device's other summation order, as in tests/test_gpu_svgp_kernels.py), never less than 1e-10 relative.  A
vector (a prediction) is one quantity: both sides of the rule are its largest entry."""
import functools

import numpy as np
import pytest

import psi_numpy as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, NS = 300, 40
SF, NOISE, EPS = 1.3, 0.3, 1e-6
ELLS = [0.9, 1.4, 1.1]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", torch.float64).contiguous()


def _within(got, v64, vld, what):
    """The module docstring's rule; prints the figures."""
    err = float(np.abs(np.asarray(got, dtype=np.longdouble) - vld).max())
    own = float(np.abs(np.asarray(v64, dtype=np.longdouble) - vld).max())
    allowed = max(10.0 * own, 1e-10 * float(np.abs(vld).max()))
    print("%s: device - longdouble %.3e, float64 - longdouble %.3e, allowed %.3e" % (what, err, own, allowed))
    return err <= allowed


@functools.lru_cache(maxsize=None)
def _problem(m, d, q, ard, zero_var=False):
    mu, s, z, y = po.problem(N, m, d, 1000 * m + 10 * d + q, q=q, far=False)
    if zero_var:
        s = np.zeros_like(s)
    ell = np.array(ELLS[:d]) if ard else 0.9
    xs = np.random.RandomState(5).randn(NS, d)
    xs_var = 10.0 ** np.random.RandomState(6).uniform(-3, 0, size=(NS, d))
    xs_var[::4] = 0.0
    m64, mld = po.both(mu, s, z, y, ell, SF, NOISE, eps=EPS)
    return mu, s, z, y, ell, xs, xs_var, m64, mld


def _block(ca, mu, var, z, ell, ard):
    from cimrgp_amd.KernelClass import RBFKernel
    if ard:
        return ca.UncertainInputBlock(_dev(mu), var, _dev(z), RBFKernel(l=1.0, sf=SF, noise=NOISE), EPS, lengthscales=ell)
    return ca.UncertainInputBlock(_dev(mu), var, _dev(z), RBFKernel(l=ell, sf=SF, noise=NOISE), EPS)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", [32, 64])
def test_block_matches_the_oracle(ca, m, d, q, ard):
    mu, s, z, y, ell, xs, xs_var, m64, mld = _problem(m, d, q, ard)
    blk = _block(ca, mu, _dev(s), z, ell, ard).fit(_dev(y))
    ok = _within(blk.bound(), m64.bound, mld.bound, "bound")
    ok &= _within(blk.kl(), m64.kl, mld.kl, "kl")
    ok &= abs(blk.elbo() - (blk.bound() - blk.kl())) == 0.0
    mean = torch.empty((NS, q), dtype=torch.float64, device="cuda")
    var = torch.empty(NS, dtype=torch.float64, device="cuda")
    blk.predict(_dev(xs), mean, var, include_noise=True)
    (a64, v64), (ald, vld) = m64.predict(xs, True), mld.predict(xs, True)
    ok &= _within(mean.cpu().numpy(), a64, ald, "mean")
    ok &= _within(var.cpu().numpy(), v64, vld, "var")
    # uncertain test inputs: the mean from Psi1*, per-row variances (the kernel) and one shared vector (the composition)
    blk.predict(_dev(xs), mean, None, xs_var=_dev(xs_var))
    ok &= _within(mean.cpu().numpy(), m64.predict_uncertain(xs, xs_var), mld.predict_uncertain(xs, xs_var), "psi1* mean (rows)")
    blk.predict(_dev(xs), mean, None, xs_var=xs_var[1], budget_bytes=1)
    ok &= _within(mean.cpu().numpy(), m64.predict_uncertain(xs, xs_var[1]), mld.predict_uncertain(xs, xs_var[1]), "psi1* mean (shared)")
    with pytest.raises(TypeError, match="not yet supported"):
        blk.predict(_dev(xs), mean, var, xs_var=0.1)
    assert ok


@pytest.mark.parametrize("m,d,q,ard", [(32, 1, 1, False), (64, 3, 2, True)])
def test_zero_variance_is_the_vfe_block(ca, m, d, q, ard):
    """x_var = 0, as a scalar (the composition) and as an (n, d) tensor of zeros (the kernels): bound() and the predictions
    are those of SparseBlock('vfe') under the rule of the module docstring."""
    from cimrgp_amd.KernelClass import RBFKernel
    mu, s, z, y, ell, xs, _, m64, mld = _problem(m, d, q, ard, zero_var=True)
    kw = dict(lengthscales=ell) if ard else {}
    vfe = ca.SparseBlock(_dev(mu), _dev(z), RBFKernel(l=1.0 if ard else ell, sf=SF, noise=NOISE), 'vfe', EPS, **kw).fit(_dev(y))
    lml = vfe.log_marginal_likelihood()
    vm, vv = torch.empty((NS, q), dtype=torch.float64, device="cuda"), torch.empty(NS, dtype=torch.float64, device="cuda")
    vfe.predict(_dev(xs), vm, vv)
    ok = _within(lml, m64.bound, mld.bound, "SparseBlock('vfe') lml")
    for var in (0.0, torch.zeros((N, d), dtype=torch.float64, device="cuda")):
        blk = _block(ca, mu, var, z, ell, ard).fit(_dev(y))
        assert blk.kl() == 0.0
        ok &= _within(blk.bound(), m64.bound, mld.bound, "bound at x_var = 0")
        ok &= abs(blk.bound() - lml) <= 2 * max(10.0 * abs(float(m64.bound - mld.bound)), 1e-10 * abs(lml))
        mean, pv = torch.empty_like(vm), torch.empty_like(vv)
        blk.predict(_dev(xs), mean, pv)
        (a64, v64), (ald, vld) = m64.predict(xs), mld.predict(xs)
        ok &= _within(mean.cpu().numpy(), a64, ald, "mean at x_var = 0") and _within(pv.cpu().numpy(), v64, vld, "var at x_var = 0")
        ok &= _within(vm.cpu().numpy(), a64, ald, "SparseBlock mean") and _within(vv.cpu().numpy(), v64, vld, "SparseBlock var")
    assert ok


def test_bad_rows_and_a_failed_factor_raise(ca):
    mu, s, z, y, ell, _, _, _, _ = _problem(32, 2, 1, False)
    sb = s.copy()
    sb[7, 0], sb[100, 1] = -1.0, np.inf
    with pytest.raises(ValueError, match="2 of the input rows"):
        _block(ca, mu, _dev(sb), z, ell, False).fit(_dev(y))
    from cimrgp_amd.KernelClass import RBFKernel
    same = np.ones((8, 2))                                       # K_uu = sf 1 1^T and no jitter: the second pivot is exactly 0
    with pytest.raises(np.linalg.LinAlgError):
        ca.UncertainInputBlock(_dev(mu), _dev(s), _dev(same), RBFKernel(l=0.9, sf=1.0, noise=NOISE), 0.0).fit(_dev(y))


# ---- the plugin ------------------------------------------------------------------------------------------------------
def _data(n, d, q, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-2.0, 3.0, size=(n, d)) * np.array([1.0, 4.0, 0.5][:d])
    y = np.sin(x @ rng.randn(d, q)) + 0.1 * rng.randn(n, q) + 2.0
    return x, y, rng.uniform(-2.0, 3.0, size=(NS, d)) * np.array([1.0, 4.0, 0.5][:d])


@functools.lru_cache(maxsize=None)
def _reference_run(n, d, q, seed):
    """The oracle run with the reference's settings: z-scored data, 100 rows drawn by RandomState(0).permutation, unit
    RBF-ARD, likelihood variance 1, X_var = inputs.var() 0.01, no optimisation."""
    x, y, xs = _data(n, d, q, seed)
    xm, xsd, ym, ysd = x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0)
    xn, yn, xsn = (x - xm) / xsd, (y - ym) / ysd, (xs - xm) / xsd
    z = xn[np.random.RandomState(0).permutation(n)[:100]]
    var = xn.var() * 0.01
    m64, mld = po.both(xn, var, z, yn, np.ones(d), 1.0, 1.0, eps=1e-6)
    return x, y, xs, (xm, xsd, ym, ysd), xsn, var, m64, mld


def test_plugin_defaults_reproduce_the_reference_settings(ca):
    n, d, q = 300, 2, 2
    x, y, xs, (xm, xsd, ym, ysd), xsn, var, m64, mld = _reference_run(n, d, q, 3)
    g = ca.BGPLVM()
    assert g.fit([x, y]) is True
    back = lambda a: np.asarray(a, dtype=np.longdouble) * ysd + ym
    (a64, v64), (ald, vld) = m64.predict(xsn), mld.predict(xsn)
    ok = _within(g.predict(xs), back(a64), back(ald), "predict")
    mean, pv = g.predict_with_variance(xs)
    ok &= _within(mean, back(a64), back(ald), "predict_with_variance mean") and _within(pv, v64, vld, "variance")
    _, pvn = g.predict_with_variance(xs, include_noise=True)
    ok &= _within(pvn, v64 + 1.0, vld + 1.0, "variance with noise")
    ok &= _within(g.elbo(), m64.elbo, mld.elbo, "elbo") and _within(g.kl_divergence(), m64.kl, mld.kl, "kl")
    assert ok
    assert list(g.lengthscales) == [1.0] * d and g.kernel.noise == 1.0 and g.kernel.sf == 1.0 and g.optimizer_result is None
    assert np.array_equal(g.inducing_ids, np.random.RandomState(0).permutation(n)[:100])
    assert np.allclose(g.inducing_inputs, x[g.inducing_ids], rtol=0, atol=1e-12)
    # uncertain test inputs, in the caller's units
    tv = np.array([0.04, 0.5])
    want64, wantld = (back(mm.predict_uncertain(xsn, tv / xsd ** 2)) for mm in (m64, mld))
    assert _within(g.predict(xs, test_var=tv), want64, wantld, "predict(test_var)")
    with pytest.raises(TypeError, match="not yet supported"):
        g.predict_with_variance(xs, test_var=tv)


def test_a_per_row_x_var_gives_what_the_equal_scalar_gives(ca):
    """X_var as a scalar takes the shared-variance route, the same value as an (n, d) array the psi kernels: one model."""
    n, d, q = 300, 2, 1
    x, y, xs = _data(n, d, q, 4)
    xsd = x.std(axis=0)
    xn, yn = (x - x.mean(axis=0)) / xsd, (y - y.mean(axis=0)) / y.std(axis=0)
    z = xn[np.random.RandomState(0).permutation(n)[:48]]
    m64, mld = po.both(xn, 0.02 / xsd ** 2, z, yn, np.ones(d), 1.0, 1.0, eps=1e-6)
    a = ca.BGPLVM(num_inducing=48, X_var=0.02)
    b = ca.BGPLVM(num_inducing=48, X_var=np.full((n, d), 0.02))
    c = ca.BGPLVM(num_inducing=48, X_var=[0.02] * d)
    for g in (a, b, c):
        g.fit([x, y])
    assert isinstance(b.block.x_var, torch.Tensor) and not isinstance(a.block.x_var, torch.Tensor)
    xsn = (xs - x.mean(axis=0)) / xsd
    back = lambda v: np.asarray(v, dtype=np.longdouble) * y.std(axis=0) + y.mean(axis=0)
    ok = True
    for g, name in ((a, "scalar"), (b, "array"), (c, "vector")):
        ok &= _within(g.elbo(), m64.elbo, mld.elbo, "elbo (%s)" % name)
        ok &= _within(g.predict(xs), back(m64.predict(xsn)[0]), back(mld.predict(xsn)[0]), "predict (%s)" % name)
    assert ok
    with pytest.raises(ValueError, match="X_var"):
        ca.BGPLVM(X_var=np.full((n - 1, d), 0.02)).fit([x, y])


def test_optimize_does_not_lower_the_bound(ca):
    x, y, xs = _data(300, 2, 1, 5)
    fixed = ca.BGPLVM(num_inducing=32)
    fixed.fit([x, y])
    learned = ca.BGPLVM(num_inducing=32, optimize=True, max_iters=5)
    learned.fit([x, y])
    print("bound: fixed %.6f, after 5 iterations %.6f" % (fixed.block.bound(), learned.block.bound()))
    assert learned.optimizer_result is not None and learned.optimizer_result.nit <= 5
    assert learned.block.bound() >= fixed.block.bound()
    assert learned.lengthscales.shape == (2,) and np.isfinite(learned.predict(xs)).all()
    # the KL term does not depend on the hyper-parameters
    assert abs(learned.kl_divergence() - fixed.kl_divergence()) <= 1e-12 * fixed.kl_divergence()


def test_plugin_serves_the_input_warp(ca):
    from cimrgp_amd.Inputs import Inputs
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(-1.0, 1.0, size=(400, 1)) ** 3, axis=0)
    xn = (x - x.mean(axis=0)) / x.std(axis=0)
    obj = Inputs(xn, ca.IndexSetUniform(400, 1, 2), learn_inputs=True, model_factory=lambda: ca.BGPLVM(num_inducing=50, noise=0.01))
    assert isinstance(obj.input_model, ca.BGPLVM)
    warped = obj.warp(xn[::7])
    assert warped.shape == (58, 1) and np.isfinite(warped).all()
