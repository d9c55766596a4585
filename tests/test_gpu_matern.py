"""The half-integer Matern covariances on the GPU: Gram / cross-Gram / fused mean / LML gradient kernels against
the closed form in NumPy (and sklearn), bit-equality of the covariance entry points with the RBF ones, the
batched layer calls, the multiresolution model and the GP_Matern plugin."""
import numpy as np
import pytest
import scipy.linalg as sla

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NUS = (0.5, 1.5, 2.5)


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=_dev(), dtype=dtype).contiguous()


# ---- NumPy restatement ------------------------------------------------------------------------------------
def _dist(xa, xb):
    d2 = np.zeros((xa.shape[0], xb.shape[0]))
    for k in range(xa.shape[1]):
        df = xa[:, k][:, None] - xb[:, k][None, :]
        d2 += df * df
    return np.sqrt(d2)


def _poly(nu, t):
    return {0.5: np.ones_like(t), 1.5: 1 + t, 2.5: 1 + t + t * t / 3}[nu]


def matern(xa, xb, nu, ell, sf, diag_add=0.0):
    t = np.sqrt(2 * nu) * _dist(xa, xb) / ell
    k = sf * _poly(nu, t) * np.exp(-t)
    if diag_add:
        k[np.diag_indices_from(k)] += diag_add
    return k


def lml_and_grad(x, y, nu, ells, sf, noise, ard):
    """LML and its gradient w.r.t. (log sf, log l (or log l_1..l_d), log noise)."""
    ells = np.broadcast_to(np.asarray(ells, dtype=np.float64), (x.shape[1],))
    xs = x / ells
    n, q = y.shape
    r = _dist(xs, xs)
    t = np.sqrt(2 * nu) * r
    v = np.exp(-t)
    kf = sf * _poly(nu, t) * v
    chol = sla.cholesky(kf + noise * np.eye(n), lower=True)
    alpha = sla.cho_solve((chol, True), y)
    lml = -0.5 * np.sum(y * alpha) - q * np.sum(np.log(np.diag(chol))) - 0.5 * n * q * np.log(2 * np.pi)
    g = alpha @ alpha.T - q * sla.cho_solve((chol, True), np.eye(n))
    grad = [0.5 * np.sum(g * kf)]
    if ard:
        c2 = 2 * nu
        with np.errstate(divide="ignore", invalid="ignore"):
            a = {0.5: np.where(r > 0, sf * v / np.where(r > 0, r, 1), 0.0), 1.5: c2 * sf * v,
                 2.5: c2 * sf * (1 + t) * v / 3}[nu]
        for k in range(x.shape[1]):
            dk = xs[:, k][:, None] - xs[:, k][None, :]
            grad.append(0.5 * np.sum(g * a * dk * dk))
    else:
        dl = {0.5: sf * t * v, 1.5: sf * t * t * v, 2.5: sf * t * t * (1 + t) * v / 3}[nu]
        grad.append(0.5 * np.sum(g * dl))
    grad.append(0.5 * noise * np.trace(g))
    return lml, np.array(grad), alpha, sla.cho_solve((chol, True), np.eye(n))


# ---- Gram / cross-Gram ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 4099])
def test_cov_gram_and_cross_match_closed_form(ca, n, d):
    dev = ca.device
    rng = np.random.default_rng(n * 10 + d)
    x = rng.uniform(-2, 2, size=(n, d))
    nb = max(1, n // 2 + 3)
    xb = rng.uniform(-2, 2, size=(nb, d))
    for nu in NUS:
        kern = ca.DenseMaternKernel(nu, l=0.6, sf=1.7)
        want = matern(x, x, nu, 0.6, 1.7, diag_add=0.05)
        want_x = matern(x, xb, nu, 0.6, 1.7)
        for dt, bar in ((torch.float64, 1e-13), (torch.float32, 2e-6)):
            xd, xbd = _t(x, dt), _t(xb, dt)
            lo = dev.rbf_gram(xd, 0.6, 1.7, 0.05, lower_only=True, cov=kern.cov)[:n, :n].double().cpu().numpy()
            assert np.max(np.abs(np.tril(lo) - np.tril(want))) / 1.7 <= bar, (nu, dt, "lower")
            full = dev.rbf_gram(xd, 0.6, 1.7, 0.05, lower_only=False, cov=kern.cov)[:n, :n].double().cpu().numpy()
            assert np.max(np.abs(full - want)) / 1.7 <= bar, (nu, dt, "full")
            cb = dev.rbf_cross(xd, xbd, 0.6, 1.7, cov=kern.cov)
            cross = cb[:n, :nb].double().cpu().numpy()
            assert np.max(np.abs(cross - want_x)) / 1.7 <= bar, (nu, dt, "cross")
            if dt == torch.float64:
                assert np.all(np.diag(full) == 1.7 + 0.05)


def test_cov_gram_matches_sklearn(ca):
    from sklearn.gaussian_process.kernels import Matern
    rng = np.random.default_rng(3)
    x = rng.normal(size=(300, 3))
    for nu in NUS:
        want = 1.3 * Matern(length_scale=0.8, nu=nu)(x)
        got = ca.DenseMaternKernel(nu, 0.8, 1.3).K(x)
        assert np.max(np.abs(got - want)) / 1.3 < 1e-13


# ---- RBF through the covariance entry points: bit-identical ------------------------------------------------
def test_cov_entry_points_with_rbf_are_bit_identical(ca):
    from cimrgp_amd import _lib
    lib = _lib.load()
    dev = ca.device
    rng = np.random.default_rng(7)
    P = dev._p
    st = dev._stream
    for dt in (torch.float64, torch.float32):
        DT = dev._DT[dt]
        for d in (1, 2, 3):
            n, ns, q = 300, 77, 2
            x, xs = _t(rng.uniform(-1, 1, (n, d)), dt), _t(rng.uniform(-1, 1, (ns, d)), dt)
            a = dev.alloc_matrix(n, n, dt, x.device).zero_()
            b = dev.alloc_matrix(n, n, dt, x.device).zero_()
            _lib.check(lib.cimrgp_rbf_gram(DT, P(x), n, d, 0.7, 1.3, 0.1, P(a), a.stride(0), 1, st()), "old")
            _lib.check(lib.cimrgp_cov_gram(DT, 0, P(x), n, d, 0.7, 1.3, 0.1, P(b), b.stride(0), 1, st()), "new")
            assert torch.equal(a, b)
            a = dev.alloc_matrix(ns, n, dt, x.device).zero_()
            b = dev.alloc_matrix(ns, n, dt, x.device).zero_()
            _lib.check(lib.cimrgp_rbf_cross(DT, P(xs), ns, P(x), n, d, 0.7, 1.3, P(a), a.stride(0), st()), "old")
            _lib.check(lib.cimrgp_cov_cross(DT, 0, P(xs), ns, P(x), n, d, 0.7, 1.3, P(b), b.stride(0), st()), "new")
            assert torch.equal(a, b)
            alpha = _t(rng.normal(size=(n, q)), dt)
            bias = _t([0.3, -0.2], dt)
            a = torch.zeros((ns, q), dtype=dt, device=x.device)
            b = torch.zeros((ns, q), dtype=dt, device=x.device)
            _lib.check(lib.cimrgp_predict_mean(DT, P(x), n, d, P(alpha), q, P(xs), ns, 0.7, 1.3, P(bias), P(a), 0, st()), "o")
            _lib.check(lib.cimrgp_cov_predict_mean(DT, 0, P(x), n, d, P(alpha), q, P(xs), ns, 0.7, 1.3, P(bias), P(b), 0,
                                                   st()), "n")
            assert torch.equal(a, b)
            kinv = dev.alloc_matrix(n, n, dt, x.device)
            kinv[:n, :n] = _t(np.eye(n) * 0.5 + 0.01, dt)
            scratch = torch.empty(lib.cimrgp_lml_grad_scratch_bytes(n) // 8, dtype=torch.float64, device=x.device)
            a = torch.empty(3, dtype=torch.float64, device=x.device)
            b = torch.empty(3, dtype=torch.float64, device=x.device)
            _lib.check(lib.cimrgp_lml_grad(DT, P(x), n, d, P(kinv), kinv.stride(0), P(alpha), q, 0.7, 1.3, 0.1, P(a),
                                           P(scratch), st()), "o")
            _lib.check(lib.cimrgp_cov_lml_grad(DT, 0, P(x), n, d, P(kinv), kinv.stride(0), P(alpha), q, 0.7, 1.3, 0.1,
                                               P(b), P(scratch), st()), "n")
            assert torch.equal(a, b)
            a = torch.empty(d + 2, dtype=torch.float64, device=x.device)
            b = torch.empty(d + 2, dtype=torch.float64, device=x.device)
            _lib.check(lib.cimrgp_lml_grad_ard(DT, P(x), n, d, P(kinv), kinv.stride(0), P(alpha), q, 1.3, 0.1, P(a),
                                               P(scratch), st()), "o")
            _lib.check(lib.cimrgp_cov_lml_grad_ard(DT, 0, P(x), n, d, P(kinv), kinv.stride(0), P(alpha), q, 1.3, 0.1,
                                                   P(b), P(scratch), st()), "n")
            assert torch.equal(a, b)
        # the batched layer calls
        outs = []
        for entry in ("old", "new"):
            outs.append(_layer_fit_predict(ca, rng_seed=11, batch=4, n=256, ns=50, d=2, dt=dt, cov=0, raw=entry))
        for u, v in zip(outs[0][:7], outs[1][:7]):
            assert torch.equal(u, v)


def _layer_fit_predict(ca, rng_seed, batch, n, ns, d, dt, cov, raw=None, ell=0.4, sf=1.2):
    """Fit ``batch`` blocks of n points and predict at ns points each; ``raw`` = 'old' / 'new' calls the C entry point
    cimrgp_layer_* / cimrgp_layer_*_cov directly (else the device wrappers).  Returns the device tensors."""
    from cimrgp_amd import _lib
    dev = ca.device
    lib = _lib.load()
    rng = np.random.default_rng(rng_seed)
    q = 2
    x = np.sort(rng.uniform(-1, 1, (batch * n, d)), axis=0)
    y = np.hstack([np.sin(3 * x[:, :1]), np.cos(2 * x[:, :1])]) + 0.1 * rng.normal(size=(batch * n, q))
    xs = np.sort(rng.uniform(-1, 1, (batch * ns, d)), axis=0)
    xd, yd, xsd = _t(x, dt), _t(y, dt), _t(xs, dt)
    device = xd.device
    starts = torch.arange(batch, dtype=torch.int64, device=device) * n
    t_starts = torch.arange(batch, dtype=torch.int64, device=device) * ns
    ld = dev.padded_ld(n)
    ws_bytes = max((dev.potrf_workspace_bytes(n, dt) + 15) // 16 * 16, 16)
    karena = torch.empty((batch, n, ld), dtype=dt, device=device)
    ws = torch.empty((batch, ws_bytes), dtype=torch.uint8, device=device)
    info = torch.zeros(batch, dtype=torch.int32, device=device)
    bias = torch.empty((batch, q), dtype=dt, device=device)
    noise = torch.empty(batch, dtype=dt, device=device)
    z = torch.empty((batch, n, q), dtype=dt, device=device)
    alpha = torch.empty((batch, n, q), dtype=dt, device=device)
    train = torch.zeros_like(yd)
    mean = torch.zeros((batch * ns, q), dtype=dt, device=device)
    var = torch.zeros(batch * ns, dtype=dt, device=device)
    if raw is None:
        dev.layer_fit(xd, yd, None, train, starts, n, ell, sf, -1.0, 0.01, 1e-8 * sf, None, None, karena, ws, info, bias,
                      noise, z, alpha, cov=cov)
        dev.layer_predict(xd, starts, n, xsd, t_starts, ns, ell, sf, karena, ws, z, bias, noise, mean, var, cov=cov)
    else:
        P, DT, st = dev._p, dev._DT[dt], dev._stream()
        ldr = dev.padded_ld(n)
        rows = torch.empty((batch, q, ldr), dtype=dt, device=device)
        scratch = torch.empty((batch, 2 * q * n), dtype=dt, device=device)
        fit_args = [P(xd), P(yd), None, P(train), P(starts), batch, n, d, q, ell, sf, -1.0, 0.01, 1e-8 * sf, None, None,
                    P(karena), karena.stride(1), karena.stride(0), P(ws), ws.stride(0), P(info), P(rows), ldr, P(z), P(alpha),
                    P(bias), P(noise), P(scratch), st]
        ldw = dev.padded_ld(n)
        w = torch.empty((batch, ns, ldw), dtype=dt, device=device)
        pred_args = [P(xd), P(starts), n, d, P(xsd), P(t_starts), ns, batch, ell, sf, P(karena), karena.stride(1),
                     karena.stride(0), P(ws), ws.stride(0), P(z), q, P(bias), P(noise), P(w), ldw, w.stride(0), P(mean),
                     P(var), st]
        if raw == "old":
            _lib.check(lib.cimrgp_layer_fit(DT, *fit_args), "cimrgp_layer_fit")
            _lib.check(lib.cimrgp_layer_predict(DT, *pred_args), "cimrgp_layer_predict")
        else:
            _lib.check(lib.cimrgp_layer_fit_cov(DT, cov, *fit_args), "cimrgp_layer_fit_cov")
            _lib.check(lib.cimrgp_layer_predict_cov(DT, cov, *pred_args), "cimrgp_layer_predict_cov")
    assert int(info.abs().max().item()) == 0
    return train, mean, var, alpha, z, bias, noise, (x, y, xs)


# ---- fused mean and LML gradient -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3])
def test_cov_predict_mean_equals_cross_gram_times_alpha(ca, d):
    dev = ca.device
    rng = np.random.default_rng(d)
    n, ns, q = 700, 333, 2
    x, xs = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (ns, d))
    alpha, bias = rng.normal(size=(n, q)), np.array([0.4, -1.1])
    for nu in NUS:
        k = ca.DenseMaternKernel(nu, 0.5, 1.4)
        got = dev.predict_mean(_t(x), _t(alpha), _t(xs), 0.5, 1.4, _t(bias), cov=k.cov).cpu().numpy()
        want = matern(xs, x, nu, 0.5, 1.4) @ alpha + bias
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-13


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", [200, 1500])
def test_cov_lml_grad_matches_analytic_and_finite_differences(ca, n, d, ard):
    dev = ca.device
    rng = np.random.default_rng(n + d)
    x = rng.uniform(-1.5, 1.5, (n, d))
    y = np.hstack([np.sin(2 * x[:, :1]), np.cos(x.sum(axis=1, keepdims=True))]) + 0.1 * rng.normal(size=(n, 2))
    ells = np.array([0.7, 1.3, 0.9][:d]) if ard else 0.8
    sf, noise = 1.1, 0.05
    for nu in NUS:
        k = ca.DenseMaternKernel(nu, 1.0, sf)
        lml, grad, alpha, kinv = lml_and_grad(x, y, nu, ells, sf, noise, ard)
        kb = dev.alloc_matrix(n, n, torch.float64, _dev())
        kb[:n, :n] = _t(kinv)
        if ard:
            got = dev.lml_grad_ard(_t(x / ells), kb, n, _t(alpha), sf, noise, cov=k.cov).cpu().numpy()
        else:
            got = dev.lml_grad(_t(x), kb, n, _t(alpha), ells, sf, noise, cov=k.cov).cpu().numpy()
        assert np.max(np.abs(got - grad)) / np.max(np.abs(grad)) < 1e-9, (nu, got, grad)
        # the plugin's whole GPU objective against central differences of the NumPy LML
        gp = ca.GP_Matern(nu=nu, ARD=ard, optimize=False)
        if ard:
            lml_g, grad_g = gp.log_marginal_likelihood_ard(_t(x), _t(y), ells, sf, noise)
            theta = np.log(np.concatenate([[sf], ells, [noise]]))
        else:
            lml_g, grad_g = gp.log_marginal_likelihood(_t(x), _t(y), ells, sf, noise)
            theta = np.log([sf, ells, noise])
        assert abs(lml_g - lml) < 1e-9 * abs(lml)

        def f(th):
            e = np.exp(th)
            return lml_and_grad(x, y, nu, e[1:-1] if ard else e[1], e[0], e[-1], ard)[0]
        h = 1e-5
        fd = np.array([(f(theta + h * np.eye(len(theta))[i]) - f(theta - h * np.eye(len(theta))[i])) / (2 * h)
                       for i in range(len(theta))])
        assert np.max(np.abs(grad_g - fd)) / np.max(np.abs(fd)) < 1e-6, (nu, grad_g, fd)


# ---- batched layers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n", [(8, 512), (4, 2048)])
def test_layer_fit_and_predict_cov_match_scipy(ca, batch, n):
    ns = 97
    for nu in NUS:
        k = ca.DenseMaternKernel(nu, 0.4, 1.2)
        train, mean, var, alpha, z, bias, noise, (x, y, xs) = _layer_fit_predict(ca, 21, batch, n, ns, 2, torch.float64,
                                                                                 k.cov)
        mean, var, train = mean.cpu().numpy(), var.cpu().numpy(), train.cpu().numpy()
        noise, bias = noise.cpu().numpy(), bias.cpu().numpy()
        for b in range(batch):
            xb, yb, xsb = x[b * n:(b + 1) * n], y[b * n:(b + 1) * n], xs[b * ns:(b + 1) * ns]
            mu = yb.mean(axis=0)
            nz = max(0.01 * np.mean((yb - mu) ** 2), 1e-8 * 1.2)
            assert abs(noise[b] - nz) < 1e-12 * nz and np.allclose(bias[b], mu, rtol=1e-13, atol=1e-15)
            kf = matern(xb, xb, nu, 0.4, 1.2)
            c = sla.cholesky(kf + nz * np.eye(n), lower=True)
            al = sla.cho_solve((c, True), yb - mu)
            ks = matern(xsb, xb, nu, 0.4, 1.2)
            m = ks @ al + mu
            v = 1.2 - np.sum(sla.solve_triangular(c, ks.T, lower=True) ** 2, axis=0) + nz
            assert np.max(np.abs(mean[b * ns:(b + 1) * ns] - m)) / np.max(np.abs(m)) < 1e-10
            assert np.max(np.abs(var[b * ns:(b + 1) * ns] - v)) / np.max(np.abs(v)) < 1e-10
            tr = kf @ al + mu
            assert np.max(np.abs(train[b * n:(b + 1) * n] - tr)) / np.max(np.abs(tr)) < 1e-10


# ---- whole model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["matern32", "mixed"])
@pytest.mark.parametrize("dtype,bar", [("f64", 1e-9), ("f32", 1e-4)])
def test_mrgp_with_matern_layers_matches_oracle_chain(ca, golden_dir, monkeypatch, case, dtype, bar):
    """Config 1 (N = 512, resolution 2, divider 2): layer 0 is one block (fitted alone), layers 1 and 2 are
    batches of equal blocks.  The oracle's chain with its Gram builder replaced by the layer's covariance.
    FP64 keeps the plugin's noise rule (1 % of the block's target variance); FP32 fixes the noise at 1, which keeps
    the condition numbers at a few hundred (the 1 % rule gives FP32 errors of 3e-2 and a non-PD block)."""
    import os
    import oracle.dense as odense
    g = np.load(os.path.join(golden_dir, "dense_oracle.npz"))
    x, y, xt = g["chain_x"], g["chain_y"], g["chain_xt"]
    n, ns, res = x.shape[0], xt.shape[0], 2
    nz = None if dtype == "f64" else 1.0
    if case == "matern32":
        kernels = [ca.DenseMaternKernel(1.5, l=1.0 / 2 ** j, sf=1.0, noise=nz) for j in range(res + 1)]
    else:
        kernels = [ca.DenseMaternKernel(0.5, l=1.0, sf=1.0, noise=nz), ca.RBFKernel(l=0.5, sf=1.0, noise=nz),
                   ca.DenseMaternKernel(2.5, l=0.25, sf=1.0, noise=nz)]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2),
                                              spectral_density_obj=kernels, dtype=dtype)
    model.fit()
    assert [len(p.batches) for p in model.posterior_obj] == [0, 1, 1]
    idx_t = ca.IndexSetUniform(ns, res, 2)
    mean = model.get_predicted_mean(xt, idx_t)
    var = model.get_central_moment2(xt, idx_t)

    by_ell = {k.l: k for k in kernels}
    rbf = odense.rbf_gram

    def gram(xa, xb=None, ell=1.0, sf2=1.0, diag_add=0.0):
        k = by_ell[ell]
        if isinstance(k, ca.DenseMaternKernel):
            return matern(xa, xa if xb is None else xb, k.nu, ell, sf2, diag_add if xb is None else 0.0)
        return rbf(xa, xb, ell, sf2, diag_add)
    monkeypatch.setattr(odense, "rbf_gram", gram)
    xn, _, mu, sd = oracle.normalize_inputs(x)
    specs = [oracle.DenseLayerSpec(k.l, k.sf, k.noise) for k in kernels]
    omodel, f_bar = oracle.mrgp_fit(xn, y, oracle.index_bounds_uniform(n, res, 2), specs)
    omean, ovar = oracle.mrgp_predict(xn, omodel, specs, (xt - mu) / sd, oracle.index_bounds_uniform(ns, res, 2))
    em = float(np.max(np.abs(mean - omean)) / np.max(np.abs(omean)))
    ev = float(np.max(np.abs(var - ovar)) / np.max(np.abs(ovar)))
    assert em < bar and ev < bar, (em, ev)


def test_snr_ratio_keeps_the_matern_class(ca):
    rng = np.random.default_rng(2)
    x = np.sort(rng.uniform(0, 1, (256, 1)), axis=0)
    y = np.hstack([np.sin(4 * x), np.cos(4 * x)]) + 0.1 * rng.normal(size=(256, 2))
    kernels = [ca.DenseMaternKernel(2.5, 1.0, 1.0), ca.DenseMaternKernel(0.5, 0.5, 1.0)]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(256, 1, 2),
                                              spectral_density_obj=kernels, snr_ratio=10.0)
    k0 = model.spectral_density_obj[0]
    assert isinstance(k0, ca.DenseMaternKernel) and (k0.nu, k0.l, k0.sf) == (2.5, 1.0, 1.0) and k0.noise > 0
    model.fit()
    assert np.all(np.isfinite(model.get_predicted_mean(x, ca.IndexSetUniform(256, 1, 2))))


# ---- GP_Matern plugin ------------------------------------------------------------------------------------------
def _plugin_data():
    rng = np.random.default_rng(5)
    n = 250
    x = np.hstack([np.sort(rng.uniform(0, 6, size=(n, 1)), axis=0), rng.uniform(-1, 1, size=(n, 1))])
    y = np.hstack([np.sin(2 * x[:, :1]), np.cos(3 * x[:, :1]) + 0.3 * x[:, 1:]]) + 0.15 * rng.normal(size=(n, 2))
    xt = np.column_stack([np.linspace(0.1, 5.9, 40), np.linspace(-0.9, 0.9, 40)])
    return x, y, xt


def test_gp_matern_fixed_matches_sklearn(ca):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    x, y, xt = _plugin_data()
    xz = (x - x.mean(0)) / x.std(0)
    yz = (y - y.mean(0)) / y.std(0)
    xtz = (xt - x.mean(0)) / x.std(0)
    for nu in NUS:
        gp = ca.GP_Matern(nu=nu, lengthscale=0.9, variance=1.3, optimize=False)
        assert gp.fit([x, y]) is True
        noise = gp.kernel.noise
        assert abs(noise - 0.01 * yz.var()) < 1e-15
        kern = ConstantKernel(1.3, "fixed") * Matern(length_scale=0.9, length_scale_bounds="fixed", nu=nu) + \
            WhiteKernel(noise, "fixed")
        sk = GaussianProcessRegressor(kern, alpha=0.0, optimizer=None, normalize_y=False).fit(xz, yz)
        m_sk, s_sk = sk.predict(xtz, return_std=True)
        s_sk = s_sk[:, 0] if s_sk.ndim == 2 else s_sk          # the same for both outputs
        m, v = gp.predict_with_variance(xt)
        assert np.max(np.abs((m - y.mean(0)) / y.std(0) - m_sk)) / np.max(np.abs(m_sk)) < 1e-9
        assert np.max(np.abs(v - (s_sk ** 2 - noise))) < 1e-9


@pytest.mark.parametrize("ard", [False, True])
def test_gp_matern_optimize_matches_scipy_on_numpy_objective(ca, ard):
    from scipy.optimize import minimize
    x, y, xt = _plugin_data()
    xz = (x - x.mean(0)) / x.std(0)
    yz = (y - y.mean(0)) / y.std(0)
    d = x.shape[1]
    for nu in NUS:
        gp = ca.GP_Matern(nu=nu, ARD=ard, optimize=True)
        gp.fit([x, y])
        noise0 = 0.01 * float(yz.var())
        theta0 = np.log([1.0] + [1.0] * (d if ard else 1) + [noise0])

        def objective(th):
            e = np.exp(th)
            try:
                lml, grad = lml_and_grad(xz, yz, nu, e[1:-1] if ard else e[1], e[0], e[-1], ard)[:2]
            except np.linalg.LinAlgError:
                return 1e100, np.zeros(len(th))
            return -lml, -grad
        res = minimize(objective, theta0, jac=True, method="L-BFGS-B", options=dict(maxiter=1000))
        e = np.exp(res.x)
        got = np.concatenate([[gp.kernel.sf], gp.lengthscales if ard else [gp.kernel.l], [gp.kernel.noise]])
        np.testing.assert_allclose(got, e, rtol=1e-5)
        assert abs(gp.optimizer_result.fun - res.fun) < 1e-8 * abs(res.fun)
        assert gp.optimizer_result.success
