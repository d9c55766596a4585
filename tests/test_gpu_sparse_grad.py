"""GPU tests of the gradients of the sparse objective (include/cimrgp_sparse_grad.h): cimrgp_cov_pair_grad,
cimrgp_sparse_grad_rows and cimrgp_sparse_grad_combine against NumPy FP64, SparseBlock.lml_grad and the plugins'
log_marginal_likelihood_grad against the autograd oracle (tests/sparse_grad_numpy.py), and the optimiser keywords.

lml_grad is tested in FP64 only: with eps = 1e-6 the condition number of K_uu + eps sf I (up to m / eps) exceeds
1 / u of FP32, so its FP32 factor is not a meaningful target for a gradient."""
import numpy as np
import pytest

import sparse_grad_numpy as sg
import sparse_numpy as sn
from grad_numpy import kcov
from test_gpu_sparse import _plugin, _plugin_inputs, _raw, _tolerance
from test_sparse_host import EPS, SETS, SF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
ELL, SF2 = 0.7, 1.3
#: (na, nb, d, same): the issue's shapes; (3001, 257, 8): 12 slices, nb no multiple of the 128-column tile, the general-d
#: instance; same: xa = xb with scale = -2 and accumulate
PAIR_SHAPES = [(1, 1, 1, False), (255, 100, 2, False), (4097, 130, 3, False), (3001, 257, 8, False), (130, 130, 2, True)]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _padded(dev, a, tdt):
    """a (rows x cols) inside a padded buffer whose padding holds NaN."""
    rows, cols = a.shape
    buf = dev.alloc_matrix(rows, cols, tdt, "cuda")
    buf.fill_(float("nan"))
    buf[:rows, :cols] = torch.as_tensor(a).to("cuda", tdt)
    return buf


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- cimrgp_cov_pair_grad --------------------------------------------------------------------------------------------
_PAIR = {}


def _pair_problem(na, nb, d, same, cov):
    """Inputs that FP32 holds exactly (one FP64 reference serves both dtypes), in [-2, 2]^d / sqrt(d) so that no
    covariance underflows in FP32 (kappa is a relative error); G of both signs spanning 1e-2 .. 1e2."""
    key = (na, nb, d, same, cov)
    if key not in _PAIR:
        rng = np.random.default_rng(na + 7 * nb + d)
        xa = _f32(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d))
        xb = xa if same else _f32(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d))
        g = _f32(rng.choice([-1.0, 1.0], size=(na, nb)) * 10.0 ** rng.uniform(-2, 2, size=(na, nb)))
        pre_s, pre_db = (_f32(rng.normal(size=2)), _f32(rng.normal(size=(nb, d)))) if same else (np.zeros(2), np.zeros((nb, d)))
        ref, mag = sg.pair_grad(xa, xb, g, cov, ELL, SF2, scale=-2.0 if same else 1.0)
        _PAIR[key] = (xa, xb, g, pre_s, pre_db, ref, mag, kcov(xa, xb, cov, ELL, SF2))
    return _PAIR[key]


PAIR_WORST = {}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("na,nb,d,same", PAIR_SHAPES)
def test_cov_pair_grad_within_the_componentwise_bound(ca, dt, cov, na, nb, d, same):
    """|err| <= ((na + 2) u + 4 kappa) sum |term| per output: the bound of a length-na sum in any order, plus the error of
    the covariance itself; kappa is the largest relative error of cimrgp_cov_cross against kcov on the same xa, xb,
    measured here, and the factor 4 covers the few more roundings of g and dk/dlog l.  With accumulate the preset value
    is one more term of the sum."""
    dev, tdt = ca.device, TDT[dt]
    xa, xb, g, pre_s, pre_db, (s_ref, db_ref), (s_mag, db_mag), k_ref = _pair_problem(na, nb, d, same, cov)
    xad, xbd = torch.as_tensor(xa).to("cuda", tdt), torch.as_tensor(xb).to("cuda", tdt)
    kappa = float((np.abs(dev.rbf_cross(xad, xbd, ELL, SF2, cov=cov)[:na, :nb].double().cpu().numpy() - k_ref) / k_ref).max())
    gbuf = _padded(dev, g, tdt)
    sums = torch.as_tensor(pre_s).to("cuda") if same else None
    db = torch.as_tensor(pre_db).to("cuda", tdt) if same else None
    sums, db = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, scale=-2.0 if same else 1.0, accumulate=same, sums=sums, db=db, cov=cov)
    s, dbh = sums.cpu().numpy(), db.double().cpu().numpy()
    factor = (na + 2) * UNIT[dt] + 4 * kappa
    rs = np.abs(s - (s_ref + pre_s)) / (factor * (s_mag + np.abs(pre_s)))
    rd = np.abs(dbh - (db_ref + pre_db)) / (factor * (db_mag + np.abs(pre_db)) + 1e-300)
    print("pair_grad %s cov %d (%d, %d, %d)%s: kappa %.2e  err/bound sums %.3e %.3e  db %.3e"
          % (dt, cov, na, nb, d, " same" if same else "", kappa, rs[0], rs[1], rd.max()))
    PAIR_WORST[dt] = max(PAIR_WORST.get(dt, 0.0), float(rs.max()), float(rd.max()))
    assert np.isfinite(s).all() and np.isfinite(dbh).all()
    assert rs.max() <= 1.0 and rd.max() <= 1.0
    # either output alone gives the same bits
    if not same:
        s_only, none = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, want_db=False, cov=cov)
        none2, db_only = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, want_sums=False, cov=cov)
        assert none is None and none2 is None
        assert torch.equal(_bits(s_only), _bits(sums)) and torch.equal(_bits(db_only), _bits(db))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cov_pair_grad_is_bit_identical_run_to_run_and_beside_other_work(ca, dt):
    dev, tdt = ca.device, TDT[dt]
    na, nb, d = 30001, 1000, 2
    rng = np.random.default_rng(11)
    xad = torch.as_tensor(rng.uniform(-2, 2, size=(na, d))).to("cuda", tdt)
    xbd = torch.as_tensor(rng.uniform(-2, 2, size=(nb, d))).to("cuda", tdt)
    gbuf = _padded(dev, rng.normal(size=(na, nb)), tdt)
    s1, d1 = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, cov=2)
    s2, d2 = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, cov=2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(d1), _bits(d2))
    # beside cimrgp_wsyrk_tn on another stream
    side = torch.cuda.Stream()
    abuf = _padded(dev, rng.normal(size=(na, nb)), tdt)
    w = torch.as_tensor(rng.uniform(0.5, 2, size=na)).to("cuda", tdt)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):
            dev.wsyrk_tn(abuf, na, nb, w)
    s3, d3 = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, cov=2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1), _bits(s3)) and torch.equal(_bits(d1), _bits(d3))


# ---- cimrgp_sparse_grad_rows / cimrgp_sparse_grad_combine ------------------------------------------------------------
def _rel_max(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m,q", [(1, 16, 1), (255, 100, 2), (4097, 1000, 8)])
def test_sparse_grad_rows_and_combine_against_numpy(ca, dt, mode, n, m, q):
    """FP64: 1e-12 relative to the largest magnitude of each output (the two sums: to the sum of magnitudes).  FP32:
    against the FP64 oracle on the values the device holds, at 4 x the FP32 error of cimrgp_sparse_tail (mean and
    variance, A* = W* = V) on the same V and gamma."""
    dev, tdt = ca.device, TDT[dt]
    rng = np.random.default_rng(n + m + q)
    rnd = (lambda *s: _f32(rng.normal(size=s))) if dt == "f32" else (lambda *s: rng.normal(size=s))
    v, a, gamma, r = rnd(n, m) / np.sqrt(m), rnd(n, m) / np.sqrt(m), rnd(m, q), rnd(n, q)
    w = 1.0 / (0.02 + rng.uniform(0, 1.3, size=n))
    noise = 0.02
    if dt == "f32":
        v, a, w = _f32(v), _f32(a), _f32(w)
    vb, ab = _padded(dev, v, tdt), _padded(dev, a, tdt)
    gd, rd, wd = (torch.as_tensor(t).to("cuda", tdt).contiguous() for t in (gamma, r, w))
    if dt == "f64":
        tol = 1e-12
    else:
        mean = torch.empty((n, q), dtype=tdt, device="cuda")
        var = torch.empty(n, dtype=tdt, device="cuda")
        dev.sparse_tail(vb, vb, n, m, gd, 1.3, 0.0, mean, var)
        tail = max(_rel_max(mean.double().cpu().numpy(), v @ gamma), _rel_max(var.double().cpu().numpy(), np.full(n, 1.3)))
        tol = 4 * tail
    beta, t, sums = dev.sparse_grad_rows(vb, n, m, gd, rd, wd, mode, noise)
    beta_ref, t_ref, h_ref = sg.rows(v, gamma, r, w, mode, noise)
    bh, th, sh = beta.double().cpu().numpy(), t.double().cpu().numpy(), sums.cpu().numpy()
    errs = (_rel_max(bh, beta_ref), _rel_max(th, t_ref), abs(sh[0] - h_ref.sum()) / np.abs(h_ref).sum(),
            abs(sh[1] - t_ref.sum()) / np.abs(t_ref).sum())
    print("grad_rows %s mode %d (%d, %d, %d): tol %.2e  beta %.2e t %.2e sum h %.2e sum t %.2e" % ((dt, mode, n, m, q, tol) + errs))
    assert max(errs) <= tol
    # combine, on the values the device holds
    b = rnd(m, q)
    y = rnd(n, m) / np.sqrt(m)
    yb = _padded(dev, y, tdt)
    dev.sparse_grad_combine(ab, yb, n, m, beta, torch.as_tensor(b).to("cuda", tdt).contiguous(), wd, t)
    ref = sg.combine(a, y, bh, b, w, th)
    err = _rel_max(yb[:n, :m].double().cpu().numpy(), ref)
    print("grad_combine %s mode %d (%d, %d, %d): %.2e" % (dt, mode, n, m, q, err))
    assert err <= tol
    assert bool(torch.isnan(yb[:n, m:]).all())


# ---- SparseBlock.lml_grad --------------------------------------------------------------------------------------------
_GRAD_REF = {}


def _grad_inputs(i):
    """Acceptance set i of tests/test_sparse_host.py (None: n = 20 000, m = 1000) with Z moved off the data: the raw
    inputs, Z in the caller's units, and what the plugin computes on."""
    n, m, d, cov, ell = SETS[i] if i is not None else (20000, 1000, 2, 0, 0.5)
    seed = 99 if i is None else i
    x, y, _ = _raw(n, d, seed)
    ids = np.random.RandomState(0).permutation(n)[:m]
    zc = x[ids] + 0.05 * x.std(axis=0) * np.random.default_rng(seed + 5).normal(size=(m, d))
    xz, _, yz, _, noise = _plugin_inputs(n, m, d, seed)
    zz = (zc - x.mean(axis=0)) / x.std(axis=0)
    return (n, m, d, cov, ell), x, y, zc, xz, zz, yz, noise


def _grad_reference(i, mode):
    """(autograd oracle, gap of the two oracle forms (theta, Z)); at n = 20 000 the gap is the worst of the four n = 1500
    sets, as for the plugin tests' tolerance."""
    if (i, mode) not in _GRAD_REF:
        (n, m, d, cov, ell), _, _, _, xz, zz, yz, noise = _grad_inputs(i)
        auto = sg.autograd(xz, zz, yz, cov, ell, SF, noise, EPS, mode)
        if i is None:
            gap = tuple(max(_grad_reference(j, mode)[1][k] for j in range(len(SETS))) for k in range(2))
        else:
            _, dth, dz, _ = sg.chain(xz, zz, yz, cov, ell, SF, noise, EPS, mode)
            gap = (sg_rel(dth, auto[1]), sg_rel(dz, auto[2]))
        _GRAD_REF[(i, mode)] = (auto, gap)
    return _GRAD_REF[(i, mode)]


def sg_rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("i", [0, 1, 2, 3, None])
def test_lml_grad_matches_the_autograd_oracle(ca, i, mode):
    """Tolerance: 100 x the gap between the two oracle forms on the same inputs, floor 1e-9 (the rule of the plugin
    tests); the value equals fit().log_marginal_likelihood() bit for bit."""
    (n, m, d, cov, ell), x, y, zc, xz, zz, yz, noise = _grad_inputs(i)
    (l_ref, th_ref, z_ref), gap = _grad_reference(i, mode)
    tol = tuple(max(1e-9, 100.0 * g) for g in gap)
    g = _plugin(ca, mode, m, cov, ell, Z=zc)
    g.fit([x, y])
    assert abs(g.kernel.noise - noise) <= 1e-15
    lml, dth, dz = g.log_marginal_likelihood_grad()
    assert lml == g.log_marginal_likelihood() == g._block(ell, SF, g.kernel.noise).fit(g._y).log_marginal_likelihood()
    blk = g._block(ell, SF, g.kernel.noise)
    lml_b, dth_b, dz_b = blk.lml_grad(g._y)
    assert lml_b == lml and np.array_equal(dth_b, dth) and np.array_equal(dz_b.cpu().numpy(), dz)
    err = (abs(lml - l_ref) / abs(l_ref), sg_rel(dth, th_ref), sg_rel(dz, z_ref))
    check = blk.grad_check
    print("lml_grad set %s mode %d: lml %.2e theta %.2e Z %.2e   tolerance %.2e %.2e   closed vs pairwise %.2e"
          % ((i, mode) + err + tol + (abs(check["closed"] - check["pairwise"]) / abs(check["closed"]),)))
    assert err[0] <= _tolerance(i, mode)[0]
    assert err[1] <= tol[0] and err[2] <= tol[1]
    # the two forms of d F / d log sf differ by the rounding of the solves with L_u: cond(K_uu + eps sf I) <= m / eps
    assert dth[0] == check["closed"] and abs(check["closed"] - check["pairwise"]) <= 2.0 ** -53 * m / EPS * abs(check["closed"])
    # theta alone: the same numbers, no dZ
    lml_t, dth_t, none = g.log_marginal_likelihood_grad(want_z=False)
    assert none is None and lml_t == lml and np.array_equal(dth_t, dth)
    # a prediction after lml_grad is the fitted block's
    if i == 1:
        xs = _raw(n, d, 1)[2]
        mean = torch.empty((xs.shape[0], 2), dtype=torch.float64, device="cuda")
        xsd = torch.as_tensor((xs - x.mean(axis=0)) / x.std(axis=0)).to("cuda")
        blk.predict(xsd, mean)
        mean2 = torch.empty_like(mean)
        g.block.predict(xsd, mean2)
        assert torch.equal(mean, mean2)


@pytest.mark.parametrize("mode", [0, 1])
def test_central_differences_of_the_device_objective(ca, mode):
    """A sanity check, not the yardstick: central differences (step 1e-4 in log theta) of the device's own
    log_marginal_likelihood agree with lml_grad to 1e-6 relative."""
    (n, m, d, cov, ell), x, y, zc, _, _, _, _ = _grad_inputs(1)
    g = _plugin(ca, mode, m, cov, ell, Z=zc)
    g.fit([x, y])
    k = g.kernel
    _, dth, _ = g.log_marginal_likelihood_grad(want_z=False)
    th0, h = np.log([k.sf, k.l, k.noise]), 1e-4
    fd = np.empty(3)
    for j in range(3):
        f = []
        for s in (h, -h):
            th = th0.copy()
            th[j] += s
            sf, el, s2 = np.exp(th)
            f.append(g.log_marginal_likelihood(el, sf, s2))
        fd[j] = (f[0] - f[1]) / (2 * h)
    print("central differences mode %d: %s against %s" % (mode, fd, dth))
    assert sg_rel(fd, dth) <= 1e-6


# ---- the optimiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_analytic_optimiser_and_learned_inducing_inputs(ca, mode):
    n, m, d = 1500, 48, 2
    x, y, xs = _raw(n, d, 21)
    xz, z0, yz, _, noise = _plugin_inputs(n, m, d, 21)
    start = sn.woodbury(xz, z0, yz, 0, 1.0, SF, noise, EPS, mode)[0]
    g = _plugin(ca, mode, m, 0, 1.0, optimize=True, jac='analytic', max_iters=8)
    g.fit([x, y])
    k = g.kernel
    end = sn.woodbury(xz, z0, yz, 0, k.l, k.sf, k.noise, EPS, mode)[0]
    print("analytic mode %d: %.6f -> %.6f in %d evaluations" % (mode, start, end, g.optimizer_result.nfev))
    assert g.optimizer_result.x.shape == (3,) and end >= start
    assert abs(g.log_marginal_likelihood() - end) <= 1e-6 * abs(end)
    assert np.allclose(g.inducing_inputs, x[g.inducing_ids], rtol=0, atol=1e-12)
    # learned Z
    gz = _plugin(ca, mode, m, 0, 1.0, optimize=True, jac='analytic', optimize_inducing=True, max_iters=8)
    gz.fit([x, y])
    kz = gz.kernel
    zl = gz._z.cpu().numpy()
    end_z = sn.woodbury(xz, zl, yz, 0, kz.l, kz.sf, kz.noise, EPS, mode)[0]
    print("learned Z mode %d: %.6f -> %.6f, Z moved by %.3f" % (mode, start, end_z, np.abs(zl - z0).max()))
    assert gz.optimizer_result.x.shape == (3 + m * d,) and end_z >= start
    assert np.array_equal(gz.optimizer_result.x[3:].reshape(m, d), zl) and np.abs(zl - z0).max() > 0
    assert abs(gz.log_marginal_likelihood() - end_z) <= 1e-6 * abs(end_z)
    # inducing_inputs: the caller's units; passed back as Z= with the learned hyper-parameters they reproduce the
    # predictions (the noise of a plain refit is the 1 % rule: the comparison goes through _block)
    assert np.allclose(gz.inducing_inputs, zl * x.std(axis=0) + x.mean(axis=0), rtol=0, atol=1e-12)
    back = (ca.SGP_FITC if mode == 0 else ca.SparseGP_RBF)(num_inducing=m, lengthscale=kz.l, variance=kz.sf, Z=gz.inducing_inputs)
    back.fit([x, y])
    assert back.optimize is False and (back.kernel.l, back.kernel.sf) == (kz.l, kz.sf)
    back.block = back._block(kz.l, kz.sf, kz.noise).fit(back._y)
    mean, var = gz.predict_with_variance(xs)
    mean_b, var_b = back.predict_with_variance(xs)
    tol = _tolerance(None, mode)
    scale = y.std(axis=0)
    print("Z passed back mode %d: mean %.2e var %.2e" % (mode, np.abs((mean - mean_b) / scale).max(), np.abs(var - var_b).max()))
    assert np.abs((mean - mean_b) / scale).max() <= tol[1] and np.abs(var - var_b).max() <= tol[2]


@pytest.mark.parametrize("mode", [0, 1])
def test_two_point_path_is_bit_equal_to_the_objective_driven_by_hand(ca, mode):
    """jac='2-point' and the default constructor: SciPy's own differences of SparseBlock.fit().log_marginal_likelihood(),
    exactly as before the analytic gradient existed."""
    from scipy.optimize import minimize
    from cimrgp_amd.Sparse import SparseBlock
    n, m, d = 800, 64, 1
    x, y, xs = _raw(n, d, 77)
    # without optimisation the default constructor is the hand-driven block; its noise is the optimiser's start
    plain = _plugin(ca, mode, m, 0, 1.0)
    plain.fit([x, y])
    noise0 = plain.kernel.noise
    hand = SparseBlock(plain._x, plain._z, plain._make_kernel(1.0, SF, noise0), plain.approximation, plain.jitter).fit(plain._y)
    assert abs(noise0 - _plugin_inputs(n, m, d, 77)[4]) <= 1e-15 and plain.log_marginal_likelihood() == hand.log_marginal_likelihood()
    assert plain.optimizer_result is None and np.allclose(plain.inducing_inputs, x[plain.inducing_ids], rtol=0, atol=1e-12)
    fits = [_plugin(ca, mode, m, 0, 1.0, optimize=True, max_iters=4, **kw) for kw in ({}, {"jac": "2-point"})]
    for g in fits:
        g.fit([x, y])
    g = fits[0]

    def objective(theta):
        sf, ell, noise = np.exp(theta)
        try:
            return -SparseBlock(g._x, g._z, g._make_kernel(float(ell), float(sf), float(noise)), g.approximation,
                                g.jitter).fit(g._y).log_marginal_likelihood()
        except np.linalg.LinAlgError:
            return 1e100

    res = minimize(objective, np.log([SF, 1.0, noise0]), jac=None, method='L-BFGS-B', options=dict(maxiter=4))
    for f in fits:
        assert np.array_equal(f.optimizer_result.x, res.x) and f.optimizer_result.nfev == res.nfev
        assert (f.kernel.sf, f.kernel.l, f.kernel.noise) == tuple(float(v) for v in np.exp(res.x))
    assert np.array_equal(fits[0].predict(xs), fits[1].predict(xs))
