"""GPU tests of the inducing-point sparse GP: cimrgp_wsyrk_tn, cimrgp_sparse_lambda and cimrgp_sparse_tail against NumPy
FP64, and the SGP_FITC / SparseGP_RBF plugins against the NumPy Woodbury form (tests/sparse_numpy.py)."""
import numpy as np
import pytest

import sparse_numpy as sn
from test_sparse_host import EPS, NOISE, SETS, SF  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
SHAPES = [(1, 16, 0), (255, 100, 2), (4097, 1000, 2), (65536, 1024, 2), (30001, 2048, 8), (8192, 4096, 1)]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


_WSYRK = {}


def _wsyrk_problem(n, m, q):
    """Inputs that FP32 holds exactly (one FP64 reference serves both dtypes); w spans 1e-2 .. 1e2."""
    key = (n, m, q)
    if key not in _WSYRK:
        _WSYRK.clear()                                  # one shape at a time: the references are large
        rng = np.random.default_rng(n + 7 * m + q)
        a = rng.normal(size=(n, m)).astype(np.float32).astype(np.float64)
        w = (10.0 ** rng.uniform(-2, 2, size=n)).astype(np.float32).astype(np.float64)
        r = rng.normal(size=(n, q)).astype(np.float32).astype(np.float64) if q else None
        _WSYRK[key] = (a, w, r) + sn.wsyrk(a, w, r, diag_add=1.0)
    return _WSYRK[key]


def _run_wsyrk(ca, a, w, r, tdt, diag_add=1.0):
    dev = ca.device
    n, m = a.shape
    abuf = dev.alloc_matrix(n, m, tdt, "cuda")
    abuf.fill_(float("nan"))
    abuf[:n, :m] = torch.as_tensor(a).to("cuda", tdt)
    wd = torch.as_tensor(w).to("cuda", tdt)
    rd = None if r is None else torch.as_tensor(r).to("cuda", tdt).contiguous()
    c, g = dev.wsyrk_tn(abuf, n, m, wd, rd, diag_add=diag_add)
    torch.cuda.synchronize()
    return c[:m, :m].clone(), g, (abuf, wd, rd)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,q", SHAPES)
def test_wsyrk_tn_within_the_componentwise_bound(ca, dt, n, m, q):
    """|err_ij| <= (n + 2) u sum_k |w_k A_ki A_kj| (diag_add counts as one more term of the diagonal's sums): the
    bound of a length-n weighted sum in any order; no slack beyond it."""
    a, w, r, c_ref, g_ref, bc, bg = _wsyrk_problem(n, m, q)
    c, g, _ = _run_wsyrk(ca, a, w, r, TDT[dt])
    c = c.double().cpu().numpy()
    il = np.tril_indices(m)
    bound = (n + 2) * UNIT[dt] * (bc + np.eye(m))
    err = np.abs(c - c_ref)
    ratio = float((err[il] / bound[il]).max())
    print("wsyrk_tn %s n=%d m=%d q=%d: max err/bound C %.3e" % (dt, n, m, q, ratio))
    assert np.isfinite(c[il]).all() and ratio <= 1.0
    if q:
        g = g.double().cpu().numpy()
        gratio = float((np.abs(g - g_ref) / ((n + 2) * UNIT[dt] * bg)).max())
        print("wsyrk_tn %s n=%d m=%d q=%d: max err/bound g %.3e" % (dt, n, m, q, gratio))
        assert np.isfinite(g).all() and gratio <= 1.0
    else:
        assert g is None


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_wsyrk_tn_is_bit_identical_run_to_run_and_beside_other_work(ca, dt):
    n, m, q = 30001, 1000, 3
    rng = np.random.default_rng(5)
    a = rng.normal(size=(n, m))
    w = 10.0 ** rng.uniform(-2, 2, size=n)
    r = rng.normal(size=(n, q))
    c1, g1, _ = _run_wsyrk(ca, a, w, r, TDT[dt])
    c2, g2, _ = _run_wsyrk(ca, a, w, r, TDT[dt])
    il = torch.tril_indices(m, m)
    bits = lambda t: t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)
    assert torch.equal(bits(c1[il[0], il[1]]), bits(c2[il[0], il[1]])) and torch.equal(bits(g1), bits(g2))
    # a concurrent stream of unrelated work (matrix products that fill the device)
    side = torch.cuda.Stream()
    x = torch.randn((4096, 4096), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            x = (x @ x) * 1e-3
    c3, g3, _ = _run_wsyrk(ca, a, w, r, TDT[dt])
    torch.cuda.synchronize()
    assert torch.equal(bits(c1[il[0], il[1]]), bits(c3[il[0], il[1]])) and torch.equal(bits(g1), bits(g3))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 1), (5, 70), (1000, 129), (20001, 1000)])
def test_sparse_lambda_against_numpy(ca, dt, mode, n, m):
    dev, tdt = ca.device, TDT[dt]
    rng = np.random.default_rng(n + m)
    a = rng.normal(size=(n, m)) * 0.5 / np.sqrt(m)
    sf2, noise = 1.3, 0.02
    if n > 4:
        a[3] *= 2.5 / np.linalg.norm(a[3])               # a planted q_3 = 6.25 > sf2 + noise
    a = a.astype(np.float32 if dt == "f32" else np.float64).astype(np.float64)
    abuf = dev.alloc_matrix(n, m, tdt, "cuda")
    abuf.fill_(float("nan"))
    abuf[:n, :m] = torch.as_tensor(a).to("cuda", tdt)
    lam, w, sums = dev.sparse_lambda(abuf, n, m, sf2, noise, mode)
    qd = (a * a).sum(axis=1)
    lam_ref = sf2 - qd + noise if mode == 0 else np.full(n, noise)
    tol = 1e-14 if dt == "f64" else 1e-6
    lam_h, w_h, s = lam.double().cpu().numpy(), w.double().cpu().numpy(), sums.cpu().numpy()
    assert np.abs(lam_h - lam_ref).max() <= tol * (sf2 + noise + qd.max())
    assert np.abs(w_h * lam_h - 1).max() <= 4 * UNIT[dt]
    bad = int((lam_ref <= 0).sum())
    assert int(s[2]) == bad and bad == (1 if (mode == 0 and n > 4) else 0)
    # the sums are FP64 sums over the stored lambda and the stored sf2 - q_i: 1e-13 relative
    if bad == 0:
        assert abs(s[0] - np.log(lam_h).sum()) <= 1e-13 * np.abs(np.log(lam_h)).sum()
    d_ref = (sf2 - qd).astype(np.float32).astype(np.float64) if dt == "f32" else sf2 - qd
    assert abs(s[1] - d_ref.sum()) <= (1e-13 if dt == "f64" else 1e-6) * np.abs(d_ref).sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ns,m,q", [(1, 1, 1), (300, 70, 2), (1000, 1000, 8)])
def test_sparse_tail_against_numpy(ca, dt, ns, m, q):
    dev, tdt = ca.device, TDT[dt]
    rng = np.random.default_rng(ns + m + q)
    rnd = lambda *s: rng.normal(size=s).astype(np.float32 if dt == "f32" else np.float64).astype(np.float64)
    a, wst, gamma = rnd(ns, m) / np.sqrt(m), rnd(ns, m) / np.sqrt(m), rnd(m, q)
    ab, wb = dev.alloc_matrix(ns, m, tdt, "cuda"), dev.alloc_matrix(ns, m, tdt, "cuda")
    for buf, v in ((ab, a), (wb, wst)):
        buf.fill_(float("nan"))
        buf[:ns, :m] = torch.as_tensor(v).to("cuda", tdt)
    gd = torch.as_tensor(gamma).to("cuda", tdt).contiguous()
    mean = torch.full((ns, q), 7.0, dtype=tdt, device="cuda")
    var = torch.full((ns,), 7.0, dtype=tdt, device="cuda")
    dev.sparse_tail(ab, wb, ns, m, gd, 1.3, 0.25, mean, var)
    tol = 1e-13 if dt == "f64" else 1e-5
    mean_ref = wst @ gamma
    var_ref = 1.3 + 0.25 - (a * a).sum(axis=1) + (wst * wst).sum(axis=1)
    assert np.abs(mean.double().cpu().numpy() - mean_ref).max() <= tol * (1 + np.abs(mean_ref).max())
    assert np.abs(var.double().cpu().numpy() - var_ref).max() <= tol * 4
    # accumulate, and either output alone
    m2, v2 = mean.clone(), var.clone()
    dev.sparse_tail(ab, wb, ns, m, gd, 1.3, 0.25, m2, None, accumulate=True)
    dev.sparse_tail(ab, wb, ns, m, None, 1.3, 0.25, None, v2, accumulate=True)
    assert torch.equal(m2, mean + mean) and torch.equal(v2, var + var)


# ---- the plugins ---------------------------------------------------------------------------------------------------
_TOL = {}


def _numpy_gap(i, mode):
    """NumPy Woodbury vs NumPy dense on acceptance set i, in the plugin's units: (lml relative, mean abs, var abs)."""
    if (i, mode) not in _TOL:
        n, m, d, cov, ell = SETS[i]
        xz, z, yz, xsz, noise = _plugin_inputs(n, m, d, i)
        lw, mw, vw = sn.woodbury(xz, z, yz, cov, ell, SF, noise, EPS, mode, xsz)
        ld, md, vd = sn.dense(xz, z, yz, cov, ell, SF, noise, EPS, mode, xsz)
        _TOL[(i, mode)] = (abs(lw - ld) / abs(ld), float(np.abs(mw - md).max()), float(np.abs(vw - vd).max()))
    return _TOL[(i, mode)]


def _tolerance(i, mode):
    """100 x the NumPy-vs-NumPy gap (our potrf rounds unlike LAPACK and cond(K_uu) ~ 1 / eps amplifies that), floor 1e-9;
    i = None: the worst of the four sets (n = 20 000, where the dense form is not run)."""
    gaps = [_numpy_gap(j, mode) for j in (range(len(SETS)) if i is None else [i])]
    return tuple(max(1e-9, 100.0 * max(g[k] for g in gaps)) for k in range(3))


def _raw(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d)) * np.arange(1, d + 1) + 3.0
    y = np.stack([np.sin(2 * x).sum(axis=1), np.cos(x).prod(axis=1)], axis=1) * 2.0 + 0.5 + 0.1 * rng.normal(size=(n, 2))
    xs = rng.uniform(-2.2, 2.2, size=(513, d)) * np.arange(1, d + 1) + 3.0
    return x, y, xs


def _plugin_inputs(n, m, d, seed):
    """What the plugin computes on, restated: z-scored inputs and labels (population std), the documented draw (seed
    0), noise = 1 % of the z-scored labels' variance."""
    x, y, xs = _raw(n, d, seed)
    mu, sd, ym, ys = x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0)
    xz, yz = (x - mu) / sd, (y - ym) / ys
    ids = np.random.RandomState(0).permutation(n)[:min(n, m)]
    return xz, xz[ids], yz, (xs - mu) / sd, float(yz.var()) * 0.01


def _plugin(ca, mode, m, cov, ell, **kw):
    cls = ca.SGP_FITC if mode == 0 else ca.SparseGP_RBF
    return cls(num_inducing=m, lengthscale=ell, variance=SF, nu={0: None, 1: 0.5, 2: 1.5, 3: 2.5}[cov], **kw)


WORST = {}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("i", [0, 1, 2, 3, None])
def test_plugins_match_the_numpy_woodbury_form(ca, i, mode):
    n, m, d, cov, ell = SETS[i] if i is not None else (20000, 1000, 2, 0, 0.5)
    seed = 99 if i is None else i
    x, y, xs = _raw(n, d, seed)
    g = _plugin(ca, mode, m, cov, ell)
    assert g.fit([x, y]) is True
    xz, z, yz, xsz, noise = _plugin_inputs(n, m, d, seed)
    assert abs(g.kernel.noise - noise) <= 1e-15 and np.array_equal(g.inducing_ids, np.random.RandomState(0).permutation(n)[:m])
    lw, mw, vw = sn.woodbury(xz, z, yz, cov, ell, SF, noise, EPS, mode, xsz)
    mean, var = g.predict_with_variance(xs)
    mean_z = (mean - y.mean(axis=0)) / y.std(axis=0)
    lml = g.log_marginal_likelihood()
    gap = (abs(lml - lw) / abs(lw), float(np.abs(mean_z - mw).max()), float(np.abs(var - vw).max()))
    tol = _tolerance(i, mode)
    print("plugin set %s mode %d: gap lml %.3e mean %.3e var %.3e   tolerance %.3e %.3e %.3e" % ((i, mode) + gap + tol))
    assert gap[0] <= tol[0] and gap[1] <= tol[1] and gap[2] <= tol[2]
    assert (var >= 0).all()
    assert np.array_equal(g.predict(xs), mean)
    # the objective at other hyper-parameters, on the same data
    l2 = g.log_marginal_likelihood(ell * 1.2, 0.9, noise * 2)
    lw2 = sn.woodbury(xz, z, yz, cov, ell * 1.2, 0.9, noise * 2, EPS, mode)[0]
    assert abs(l2 - lw2) <= tol[0] * abs(lw2)
    _, var_noisy = g.predict_with_variance(xs, include_noise=True)
    assert np.abs(var_noisy - var - noise).max() <= 1e-14


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_prediction_is_bit_equal(ca, mode):
    n, m, d, cov, ell = SETS[1]
    x, y, _ = _raw(n, d, 1)
    xs = np.random.default_rng(8).uniform(-2.2, 2.2, size=(3001, d)) * np.arange(1, d + 1) + 3.0
    g = _plugin(ca, mode, m, cov, ell)
    g.fit([x, y])
    assert g.block.chunk_rows(1) == 256 and g.block.chunk_rows() > 3001
    mean, var = g.predict_with_variance(xs)
    mean_c, var_c = g.predict_with_variance(xs, budget_bytes=1)          # 256 rows at a time: 12 chunks
    assert np.array_equal(mean, mean_c) and np.array_equal(var, var_c)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [1, 2])
def test_inducing_at_the_data_gives_the_exact_plugin(ca, d, mode):
    """Z = X, eps = 0, Matern 1/2: the GP_Matern(0.5, optimize=False) prediction, within the plugins' tolerance."""
    x, y, xs = _raw(600, d, 40 + d)
    g = _plugin(ca, mode, 600, 1, 1.0, Z=x, jitter=0.0)
    g.fit([x, y])
    e = ca.GP_Matern(0.5, optimize=False)
    e.fit([x, y])
    mean, var = g.predict_with_variance(xs)
    emean, evar = e.predict_with_variance(xs)
    tol = _tolerance(None, mode)
    scale = y.std(axis=0)
    print("Z = X d=%d mode %d: mean %.3e var %.3e" % (d, mode, np.abs((mean - emean) / scale).max(), np.abs(var - evar).max()))
    assert np.abs((mean - emean) / scale).max() <= tol[1] and np.abs(var - evar).max() <= tol[2]


@pytest.mark.parametrize("mode", [0, 1])
def test_optimize_does_not_lower_the_objective(ca, mode):
    n, m, d = 800, 64, 1
    x, y, _ = _raw(n, d, 77)
    g = _plugin(ca, mode, m, 0, 1.0, optimize=True, max_iters=15)
    g.fit([x, y])
    xz, z, yz, _, noise = _plugin_inputs(n, m, d, 77)
    start = sn.woodbury(xz, z, yz, 0, 1.0, SF, noise, EPS, mode)[0]
    k = g.kernel
    end = sn.woodbury(xz, z, yz, 0, k.l, k.sf, k.noise, EPS, mode)[0]
    print("optimize mode %d: %.6f -> %.6f at l %.4f sf %.4f noise %.5f" % (mode, start, end, k.l, k.sf, k.noise))
    assert g.optimizer_result is not None and end >= start
    assert abs(g.log_marginal_likelihood() - end) <= 1e-6 * abs(end)


def test_adaptive_inputs_model_takes_a_fitted_sparse_plugin(ca):
    rng = np.random.default_rng(3)
    n, ns, res = 6000, 500, 2
    x = np.sort(rng.uniform(1, 3, size=(n, 1)) ** 2, axis=0)
    y = np.hstack([np.sin(2 * x), np.cos(x)]) + 0.05 * rng.normal(size=(n, 2))
    xs = np.sort(rng.uniform(1.5, 8.5, size=(ns, 1)), axis=0)
    xn = (x - x.mean(axis=0)) / x.std(axis=0)
    grid = np.linspace(xn.min(), xn.max(), n)[:, None]
    warp = ca.SGP_FITC(num_inducing=200, lengthscale=0.3)
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
    obj = Inputs(xn[:2000], ca.IndexSetUniform(2000, 1, 2), learn_inputs=True,
                 model_factory=lambda: ca.SGP_FITC(num_inducing=100, lengthscale=0.3))
    assert isinstance(obj.input_model, ca.SGP_FITC) and np.isfinite(obj.warp(xsn)).all()
