"""GPU tests of the variational sparse GP (cimrgp_amd/SVGP.py, the SVIGP_RBF plugin; DESIGN.md, "Variational sparse GP with a
Student-t likelihood"), FP64.  Block level: SVGPBlock.elbo_grad and predict against the oracle of tests/svgp_numpy.py at a
perturbed (mu, P), and against SparseBlock('vfe') at the Gaussian optimum.  Plugin: SVIGP_RBF's gradient against central
differences of its own objective, its robustness to outliers, and its use as the model's input warp.

The bound of every comparison with the oracle is the project's standing rule: 100 x the oracle's own dense-against-chain
gap on the same inputs, floor 1e-9, per vector relative to its largest entry."""
import numpy as np
import pytest

import svgp_numpy as so

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, M, NS = 600, 64, 300
SF, S2, NU, WHITE, EPS = 1.3, 0.05, 3.0, 0.01, 1e-6
ELLS, LINS = np.array([0.7, 1.3, 0.9]), np.array([0.5, 0.2, 0.35])
ARMS = ["plain", "ard", "ard_linear"]
_CASES = {}


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


def _gap(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _tol(a, b):
    return max(100 * _gap(a, b), 1e-9)


def _case(d, q, cov, arm, lik):
    """The inputs and the oracle's two forms, computed once per case and left unchanged."""
    key = (d, q, cov, arm, lik)
    if key not in _CASES:
        x, z, y = so.problem(N, M, d, q, 10 * d + q)
        xs = np.random.default_rng(5).uniform(-1.1, 1.1, size=(NS, d))
        ell = 0.8 if arm == "plain" else ELLS[:d]
        lin = LINS[:d] if arm == "ard_linear" else None
        theta = so.theta_of(ell, SF, S2, lin)
        mu, p = so.perturbed_posterior(M, q, 3)
        kw = dict(white=WHITE, eps=EPS, linear=lin is not None)
        _CASES[key] = dict(x=x, z=z, y=y, xs=xs, ell=ell, lin=lin, theta=theta, mu=mu, p=p, kw=kw,
                           dense=so.elbo("dense", x, z, y, cov, theta, mu, p, lik, nu=NU, **kw),
                           chain=so.elbo("chain", x, z, y, cov, theta, mu, p, lik, nu=NU, **kw),
                           pdense=so.predict("dense", x, z, xs, cov, theta, mu, p, **kw),
                           pchain=so.predict("chain", x, z, xs, cov, theta, mu, p, **kw),
                           minv=so.min_variance(x, z, cov, theta, mu, p, **kw))
    return _CASES[key]


def _kernel(ca, cov, ell, sf):
    return ca.RBFKernel(l=ell, sf=sf) if cov == 0 else ca.DenseMaternKernel(nu=cov - 0.5, l=ell, sf=sf)


def _block(ca, c, cov, lik, white=WHITE, scale=S2):
    ard = np.ndim(c["ell"]) > 0
    return ca.SVGPBlock(_dev(c["x"]), _dev(c["z"]), _kernel(ca, cov, 1.0 if ard else c["ell"], SF), lik, NU, scale, white, EPS,
                        lengthscales=c["ell"] if ard else None, linear=c["lin"])


@pytest.mark.parametrize("lik", ["gaussian", "student_t"])
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_block_objective_gradient_and_prediction_against_the_oracle(ca, d, q, cov, arm, lik):
    c = _case(d, q, cov, arm, lik)
    assert c["minv"] > 0                                  # no case is skipped: the oracle's latent variances are positive
    (fd, td, md, pd), (fc, tc, mc, pc) = c["dense"], c["chain"]
    blk = _block(ca, c, cov, lik)
    mu, p = _dev(c["mu"]), _dev(c["p"])
    f, dth, dmu, dp = blk.elbo_grad(_dev(c["y"]), mu, p)
    f2, dth2, dmu2, dp2 = _block(ca, c, cov, lik).elbo_grad(_dev(c["y"]), mu, p)
    assert f == f2 and np.array_equal(dth, dth2) and torch.equal(dmu, dmu2) and torch.equal(dp, dp2)   # run to run
    assert dth.shape == c["theta"].shape and tuple(dmu.shape) == (q, M) and tuple(dp.shape) == (q, M, M)
    assert bool((torch.triu(dp, 1) == 0).all())
    tol_f = max(100 * abs(fc - fd) / abs(fd), 1e-9)
    gf = abs(f - fd) / abs(fd)
    gt, gm, gp = _gap(dth, td), _gap(dmu.cpu().numpy(), md), _gap(dp.cpu().numpy(), pd)
    tt, tm, tp = _tol(tc, td), _tol(mc, md), _tol(pc, pd)
    mean = torch.full((NS, q), float("nan"), dtype=torch.float64, device="cuda")
    var = torch.full((NS, q), float("nan"), dtype=torch.float64, device="cuda")
    blk.set_posterior(mu, p).predict(_dev(c["xs"]), mean, var, budget_bytes=1 << 17)          # several chunks
    (dm, dv), (cm, cv) = c["pdense"], c["pchain"]
    gpm, gpv = _gap(mean.cpu().numpy(), dm), _gap(var.cpu().numpy(), dv)
    tpm, tpv = _tol(cm, dm), _tol(cv, dv)
    print("svgp d %d q %d cov %d %s %s: F %.2e (tol %.2e) theta %.2e (%.2e) mu %.2e (%.2e) P %.2e (%.2e) mean %.2e (%.2e) var %.2e"
          " (%.2e)" % (d, q, cov, arm, lik, gf, tol_f, gt, tt, gm, tm, gp, tp, gpm, tpm, gpv, tpv))
    assert gf <= tol_f and gt <= tt and gm <= tm and gp <= tp
    assert gpm <= tpm and gpv <= tpv


@pytest.mark.parametrize("arm", ARMS)
def test_chunked_prediction_is_bit_equal_to_unchunked(ca, arm):
    c = _case(2, 2, 0, arm, "student_t")
    blk = _block(ca, c, 0, "student_t").set_posterior(_dev(c["mu"]), _dev(c["p"]))
    assert blk.chunk_rows(1 << 17) < NS <= blk.chunk_rows()
    outs = []
    for budget in (None, 1 << 17):
        mean = torch.full((NS, 2), float("nan"), dtype=torch.float64, device="cuda")
        var = torch.full((NS, 2), float("nan"), dtype=torch.float64, device="cuda")
        blk.predict(_dev(c["xs"]), mean, var, budget_bytes=budget)
        outs.append((mean, var))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    only_mean = torch.empty((NS, 2), dtype=torch.float64, device="cuda")
    blk.predict(_dev(c["xs"]), only_mean, None)
    assert torch.equal(only_mean, outs[0][0])


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("q", [1, 2])
def test_at_the_gaussian_optimum_the_bound_and_its_gradient_are_the_vfe_fits(ca, q, cov, arm):
    """White variance 0, Gaussian likelihood, P = L_B and mu = L_B^-T gamma of the VFE fit with noise s2: F is the VFE bound,
    dF/dtheta its gradient (the posterior's share vanishes) and dF/d(mu, P) = 0.  Bound: the standing rule, with the
    oracle's gap of the same case; the zero gradient is held to that bound times the perturbed case's gradient scale."""
    c = _case(2, q, cov, arm, "gaussian")
    kw = dict(c["kw"], white=0.0)
    mu, p = so.gaussian_optimum(c["x"], c["z"], c["y"], cov, c["theta"], **kw)
    fd = so.elbo("dense", c["x"], c["z"], c["y"], cov, c["theta"], mu, p, "gaussian", **kw)
    fc = so.elbo("chain", c["x"], c["z"], c["y"], cov, c["theta"], mu, p, "gaussian", **kw)
    ard = np.ndim(c["ell"]) > 0
    y = _dev(c["y"])
    kern = _kernel(ca, cov, 1.0 if ard else c["ell"], SF)
    kern.noise = S2
    vfe = ca.SparseBlock(_dev(c["x"]), _dev(c["z"]), kern, "vfe", EPS, lengthscales=c["ell"] if ard else None, linear=c["lin"])
    lml, dth_vfe, _ = vfe.lml_grad(y, want_z=False)
    assert lml == vfe.log_marginal_likelihood()
    f, dth, dmu, dp = _block(ca, c, cov, "gaussian", white=0.0).elbo_grad(y, _dev(mu), _dev(p))
    tol_f, tol_t = max(100 * abs(fc[0] - fd[0]) / abs(fd[0]), 1e-9), _tol(fc[1], fd[1])
    scale_mu, scale_p = np.abs(c["dense"][2]).max(), np.abs(c["dense"][3]).max()
    zm, zp = float(dmu.abs().max()) / scale_mu, float(dp.abs().max()) / scale_p
    print("gaussian optimum q %d cov %d %s: F vs VFE %.2e (tol %.2e) theta %.2e (%.2e) |dmu| %.2e |dP| %.2e; oracle |dmu| %.2e |dP| %.2e"
          % (q, cov, arm, abs(f - lml) / abs(lml), tol_f, _gap(dth, dth_vfe), tol_t, zm, zp,
             np.abs(fd[2]).max() / scale_mu, np.abs(fd[3]).max() / scale_p))
    assert abs(f - lml) <= tol_f * abs(lml) and abs(f - fd[0]) <= tol_f * abs(fd[0])
    assert _gap(dth, dth_vfe) <= tol_t and _gap(dth, fd[1]) <= tol_t
    assert zm <= max(100 * np.abs(fd[2]).max() / scale_mu, 1e-9) and zp <= max(100 * np.abs(fd[3]).max() / scale_p, 1e-9)


def test_failures_raise_linalgerror_and_float32_is_refused(ca):
    c = _case(1, 1, 0, "plain", "student_t")
    blk = _block(ca, c, 0, "student_t")
    p = c["p"].copy()
    p[0, 5, :] = 0.0                                      # a singular P: P P^T is not positive definite
    with pytest.raises(np.linalg.LinAlgError):
        blk.elbo_grad(_dev(c["y"]), _dev(c["mu"]), _dev(p))
    with pytest.raises(np.linalg.LinAlgError):
        blk.set_posterior(_dev(c["mu"]), _dev(p))
    with pytest.raises(TypeError, match="not yet supported"):
        ca.SVGPBlock(_dev(c["x"]).float(), _dev(c["z"]).float(), ca.RBFKernel(l=1.0, sf=1.0))
    with pytest.raises(ValueError):
        blk.elbo_grad(_dev(c["y"]), _dev(c["mu"])[:, :5], _dev(c["p"]))


# ---- the plugin ------------------------------------------------------------------------------------------------------
def _plugin_data(n, d, q, seed):
    x, _, y = so.problem(n, 8, d, q, seed)
    return 2.0 * x + 0.5, 3.0 * y - 1.0


@pytest.mark.parametrize("lik,ard,linear", [("student_t", True, True), ("gaussian", False, False)])
def test_plugin_gradient_against_central_differences_of_its_own_objective(ca, lik, ard, linear):
    """Central differences (step 1e-5) of SVIGP_RBF.elbo over every hyper-parameter and a spread of the entries of mu and
    vech(P), diagonal ones included.  Bound: 10 x the gap the oracle's own central differences show against its autograd
    at the same z-scored data and parameters, relative to the largest gradient entry."""
    x, y = _plugin_data(160, 2, 2, 4)
    gp = ca.SVIGP_RBF(num_inducing=12, likelihood=lik, optimize=True, max_iters=5, ARD=ard, linear=linear)
    assert gp.fit([x, y]) is True
    f, grad = gp.elbo_grad()
    assert f == gp.elbo() and grad.shape == gp.params.shape
    nt, m, q = gp._n_theta, 12, 2
    tri = m * (m + 1) // 2
    diag = np.cumsum(np.arange(1, m + 1)) - 1             # positions of the diagonal in a row-major lower triangle
    idx = np.concatenate([np.arange(nt), nt + np.arange(0, q * m, 5), nt + q * m + diag[::3], nt + q * m + tri + diag[1::4],
                          nt + q * m + np.arange(2, 2 * tri, 17)])
    idx = np.unique(idx)
    step, cd = 1e-5, np.empty(idx.size)
    for j, k in enumerate(idx):
        hi, lo = gp.params.copy(), gp.params.copy()
        hi[k] += step
        lo[k] -= step
        cd[j] = (gp.elbo(hi) - gp.elbo(lo)) / (2 * step)
    # the oracle at the same point, in the same coordinates
    from cimrgp_amd import Hyper
    xn, yn = (x - x.mean(0)) / x.std(0), (y - y.mean(0)) / y.std(0)
    z = xn[gp.inducing_ids]
    kw = dict(nu=3.0, white=0.01, eps=1e-6, linear=linear)

    def oracle(vec, grad):
        mu, p = Hyper.unpack_posterior(vec[nt:], q, m)
        out = so.elbo("chain", xn, z, yn, 0, vec[:nt], mu, p, lik, grad=grad, **kw)
        return out[0] if not grad else (out[0], np.concatenate([out[1], Hyper.posterior_gradient(out[2], out[3], p)]))

    of, ograd = oracle(gp.params, True)
    ocd = np.empty(idx.size)
    for j, k in enumerate(idx):
        hi, lo = gp.params.copy(), gp.params.copy()
        hi[k] += step
        lo[k] -= step
        ocd[j] = (oracle(hi, False) - oracle(lo, False)) / (2 * step)
    scale = np.abs(ograd).max()
    oracle_gap = float(np.abs(ocd - ograd[idx]).max() / scale)
    got = float(np.abs(cd - grad[idx]).max() / scale)
    print("plugin %s: F %.6f (oracle %.6f) central differences %.2e (oracle's %.2e), analytic vs oracle %.2e"
          % (lik, f, of, got, oracle_gap, _gap(grad, ograd)))
    assert abs(f - of) <= 1e-9 * abs(of) and _gap(grad, ograd) <= 1e-9
    assert got <= 10 * oracle_gap


def test_plugin_interface_and_refusals(ca):
    x, y = _plugin_data(200, 2, 2, 6)
    gp = ca.SVIGP_RBF(num_inducing=16, optimize=True, max_iters=10)
    with pytest.raises(RuntimeError):
        gp.elbo()
    assert gp.fit([x, y]) is True
    assert gp.name == "SVIGP_RBF" and gp.lengthscales.shape == (2,) and gp.linear_variances.shape == (2,)
    assert gp.likelihood_scale > 0 and gp.optimizer_result is not None and gp.inducing_inputs.shape == (16, 2)
    start = ca.SVIGP_RBF(num_inducing=16, optimize=False)
    start.fit([x, y])
    assert gp.elbo() > start.elbo() and abs(start.likelihood_scale - 0.01) <= 1e-16 and start.optimizer_result is None
    xs = x[:50] + 0.01
    mean, var = gp.predict_with_variance(xs, budget_bytes=1 << 14)
    assert mean.shape == (50, 2) and var.shape == (50, 2) and (var > 0).all()
    assert np.array_equal(gp.predict(xs), mean)
    # the z-scoring, against the oracle at the fitted parameters
    from cimrgp_amd import Hyper
    xn, yn = (x - x.mean(0)) / x.std(0), (y - y.mean(0)) / y.std(0)
    mu, p = Hyper.unpack_posterior(gp.params[gp._n_theta:], 2, 16)
    args = (xn, xn[gp.inducing_ids], (xs - x.mean(0)) / x.std(0), 0, gp.params[:gp._n_theta], mu, p)
    (cm, cv), (dm, dv) = so.predict("chain", *args, linear=True), so.predict("dense", *args, linear=True)
    assert _gap(mean, dm * y.std(0) + y.mean(0)) <= _tol(cm, dm) and _gap(var, dv) <= _tol(cv, dv)
    for call in (lambda: gp.predictive_gradients(xs), lambda: gp.leave_one_out(), lambda: gp.loo_log_predictive_density(),
                 lambda: gp.predict_with_covariance(xs), lambda: gp.posterior_samples_f(xs)):
        with pytest.raises(TypeError, match="not yet supported"):
            call()


def outlier_problem():
    """y = sin 3x + 0.1 noise on 600 points, every 17th target shifted by +3: (x, y, the noise-free curve)."""
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(-1.0, 1.0, size=(600, 1)), axis=0)
    clean = np.sin(3.0 * x)
    y = clean + 0.1 * rng.normal(size=(600, 1))
    y[::17] += 3.0
    return x, y, clean


def test_student_t_fit_is_closer_to_the_clean_curve_than_the_gaussian_fit(ca):
    x, y, clean = outlier_problem()
    rmse = {}
    for lik in ("student_t", "gaussian"):
        gp = ca.SVIGP_RBF(num_inducing=40, likelihood=lik, max_iters=50)
        gp.fit([x, y])
        rmse[lik] = float(np.sqrt(np.mean((gp.predict(x) - clean) ** 2)))
        print("outliers, %s: RMSE against the noise-free curve %.4f, scale %.4g, bound %.3f" % (lik, rmse[lik], gp.likelihood_scale, gp.elbo()))
    assert rmse["student_t"] < rmse["gaussian"]


def test_plugin_as_the_input_warp_of_a_small_model(ca):
    rng = np.random.default_rng(3)
    n, ns, res = 800, 100, 1
    x = np.sort(rng.uniform(1, 3, size=(n, 1)) ** 2, axis=0)
    y = np.hstack([np.sin(2 * x), np.cos(x)]) + 0.05 * rng.normal(size=(n, 2))
    xs = np.sort(rng.uniform(1.5, 8.5, size=(ns, 1)), axis=0)
    xn = (x - x.mean(axis=0)) / x.std(axis=0)
    grid = np.linspace(xn.min(), xn.max(), n)[:, None]
    warp = ca.SVIGP_RBF(num_inducing=20, max_iters=20)
    warp.fit([xn, grid])
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2),
                                              spectral_density_obj=ca.RBFKernel(l=0.3, sf=1.0), adaptive_inputs=True,
                                              input_model=warp)
    assert model.input_obj.input_model is warp
    model.fit()
    mean = model.get_predicted_mean(xs, ca.IndexSetUniform(ns, res, 2))
    assert mean.shape == (ns, 2) and np.isfinite(mean).all()
    xsn = (xs - x.mean(axis=0)) / x.std(axis=0)
    assert np.array_equal(model.input_obj.warp(xsn), warp.predict(xsn))
    # and a factory of the plugin serves Inputs' own fit
    from cimrgp_amd.Inputs import Inputs
    obj = Inputs(xn[:400], ca.IndexSetUniform(400, 1, 2), learn_inputs=True,
                 model_factory=lambda: ca.SVIGP_RBF(num_inducing=16, max_iters=10))
    assert isinstance(obj.input_model, ca.SVIGP_RBF) and np.isfinite(obj.warp(xsn)).all()
