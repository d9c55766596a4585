"""GPU tests of the sparse GP's posterior queries (include/cimrgp_sparse_post.h; DESIGN.md, "Posterior queries of the sparse
GP"): the four entry points against NumPy at their componentwise bounds, then SparseBlock.predict_grad / loo / joint and the
plugins' five methods against the oracle of tests/sparse_post_numpy.py."""
import numpy as np
import pytest

import sparse_ard_numpy as sa
import sparse_post_numpy as sp
from test_sparse_post_host import CENTRAL_LEVEL, MARGIN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
#: (ns, m, d, q): one row; ragged 128-tiles; m one past a tile; the largest d and q
SHAPES = [(1, 16, 1, 1), (255, 100, 2, 2), (600, 257, 3, 2), (257, 1000, 8, 8)]
ELL, SF, NOISE, EPS = 0.7, 1.3, 0.02, 1e-6
#: roundings a derivative slab's element may be off its extended-precision value: 10 x the 36.2 that FP64 NumPy spends on
#: the same expression against numpy.longdouble over these shapes and the four covariances (measured once, on the host)
D_ROUNDINGS = 362.0


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _round(a, dt):
    return np.asarray(a, dtype=np.float32 if dt == "f32" else np.float64).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", TDT[dt]).contiguous()


def _padded(ca, a, dt, ld=None):
    """a (rows x cols) inside a NaN-filled buffer of padded pitch."""
    rows, cols = a.shape
    ld = ca.device.padded_ld(cols) if ld is None else ld
    buf = torch.full((rows, ld), float("nan"), dtype=TDT[dt], device="cuda")
    buf[:, :cols] = _dev(a, dt)
    return buf


def _slabs(ca, a, dt):
    """a (s, rows, cols) as back-to-back NaN-padded slabs."""
    s, rows, cols = a.shape
    ld = ca.device.padded_ld(cols)
    buf = torch.full((s, rows, ld), float("nan"), dtype=TDT[dt], device="cuda")
    buf[:, :, :cols] = _dev(a, dt)
    return buf


def _points(ns, m, d, dt, seed):
    rng = np.random.default_rng(seed)
    xb = _round(rng.uniform(-2, 2, size=(m, d)) / np.sqrt(d), dt)
    xa = _round(rng.uniform(-2, 2, size=(ns, d)) / np.sqrt(d), dt)
    k = min(ns, m) // 2 + 1
    xa[:k] = xb[:k]                                      # pairs at r = 0
    return xa, xb, k


# ---- cimrgp_cov_cross_grad ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_cov_cross_grad_slab0_is_cov_cross_and_the_derivative_slabs_are_within_roundings(ca, dt, cov, ns, m, d, q):
    dev = ca.device
    xa, xb, k = _points(ns, m, d, dt, ns + m + d + cov)
    xad, xbd = _dev(xa, dt), _dev(xb, dt)
    ld = dev.padded_ld(m)
    out = torch.full((d + 1, ns, ld), float("nan"), dtype=TDT[dt], device="cuda")
    dev.cov_cross_grad(xad, xbd, ELL, SF, out, cov=cov)
    kref = dev.rbf_cross(xad, xbd, ELL, SF, cov=cov)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[0, :, :m]), _bits(kref[:ns, :m]))
    assert bool(torch.isnan(out[:, :, m:]).all())        # padding columns are not written
    _, gl, dfl = sa.k_and_g(xa, xb, cov, ELL, SF, np.longdouble)
    ref = np.moveaxis(np.asarray(-gl[:, :, None] * dfl, dtype=np.float64), 2, 0)
    got = out[1:, :, :m].double().cpu().numpy()
    err = np.abs(got - ref)
    bound = D_ROUNDINGS * UNIT[dt] * np.abs(ref)
    worst = float((err / (UNIT[dt] * np.abs(ref) + 1e-300)).max())
    print("cov_cross_grad %s cov %d %s: worst %.1f roundings" % (dt, cov, (ns, m, d), worst))
    assert np.isfinite(got).all() and (err <= bound).all()
    idx = np.arange(k)
    assert (got[:, idx, idx] == 0).all()                 # x* = z_j: the difference is 0, and Matern 1/2's g is 0 there


# ---- cimrgp_sparse_tail_grad -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_tail_grad_within_the_componentwise_bound(ca, dt, ns, m, d, q):
    """|err| <= (m + 2) u sum |terms| for both outputs (the terms of var_grad: 2 W dW and 2 A dA); accumulate adds in the
    dtype; either output alone, and a row on its own, give the same bits."""
    dev = ca.device
    rng = np.random.default_rng(ns + m + d + q)
    a = _round(rng.normal(size=(d + 1, ns, m)), dt)
    w = _round(rng.normal(size=(d + 1, ns, m)), dt)
    gamma = _round(rng.normal(size=(m, q)), dt)
    ad, wd, gd = _slabs(ca, a, dt), _slabs(ca, w, dt), _dev(gamma, dt)
    mg = torch.full((ns, d, q), float("nan"), dtype=TDT[dt], device="cuda")
    vg = torch.full((ns, d), float("nan"), dtype=TDT[dt], device="cuda")
    dev.sparse_tail_grad(ad, wd, ns, m, gd, mg, vg)
    torch.cuda.synchronize()
    mref, vref, mmag, vmag = sp.tail_grad(a, w, gamma)
    rm = float((np.abs(mg.double().cpu().numpy() - mref) / ((m + 2) * UNIT[dt] * mmag)).max())
    rv = float((np.abs(vg.double().cpu().numpy() - vref) / ((m + 2) * UNIT[dt] * vmag)).max())
    print("sparse_tail_grad %s %s: max err/bound mean %.3e var %.3e" % (dt, (ns, m, d, q), rm, rv))
    assert rm <= 1.0 and rv <= 1.0
    m2, v2 = torch.full_like(mg, float("nan")), torch.full_like(vg, float("nan"))
    dev.sparse_tail_grad(None, wd, ns, m, gd, m2, None)
    dev.sparse_tail_grad(ad, wd, ns, m, None, None, v2)
    assert torch.equal(_bits(m2), _bits(mg)) and torch.equal(_bits(v2), _bits(vg))
    dev.sparse_tail_grad(ad, wd, ns, m, gd, m2, v2, accumulate=True)
    assert torch.equal(_bits(m2), _bits(mg + mg)) and torch.equal(_bits(v2), _bits(vg + vg))
    # the last row alone (ns = 1): the same bits
    r = ns - 1
    m1, v1 = torch.empty((1, d, q), dtype=TDT[dt], device="cuda"), torch.empty((1, d), dtype=TDT[dt], device="cuda")
    dev.sparse_tail_grad(_slabs(ca, a[:, r:r + 1], dt), _slabs(ca, w[:, r:r + 1], dt), 1, m, gd, m1, v1)
    assert torch.equal(_bits(m1[0]), _bits(mg[r])) and torch.equal(_bits(v1[0]), _bits(vg[r]))


# ---- cimrgp_sparse_loo -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_loo_within_the_propagated_bound(ca, dt, mode, ns, m, d, q):
    """The three sums of a row (q_i, |V_i|^2, V_i gamma) each carry at most (m + 2) u sum |terms|; to first order that is
    d lambda <= dq, d h <= ds / lambda + h dlambda / lambda, and
    d loo_var <= dlambda / (1 - h) + lambda dh / (1 - h)^2, d loo_mean <= dmu / (1 - h) + |r - mu| dh / (1 - h)^2,
    plus 4 u of the result for the closing scalar operations and the rounding to the dtype.  A planted row with h > 1 is
    counted, in every call anew."""
    dev = ca.device
    rng = np.random.default_rng(ns + m + q + mode)
    a = _round(rng.normal(size=(ns, m)) * 0.5 / np.sqrt(m), dt)
    v = _round(rng.normal(size=(ns, m)) * 0.05 / np.sqrt(m), dt)
    planted = ns > 4
    if planted:
        v[3] = _round(v[3] * (3.0 / np.linalg.norm(v[3])), dt)          # |V_3|^2 = 9 > lambda
    gamma = _round(rng.normal(size=(m, q)), dt)
    r = _round(rng.normal(size=(ns, q)), dt)
    ad, vd = _padded(ca, a, dt), _padded(ca, v, dt)
    lm = torch.full((ns, q), float("nan"), dtype=TDT[dt], device="cuda")
    lv = torch.full((ns,), float("nan"), dtype=TDT[dt], device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev.sparse_loo(ad, vd, ns, m, _dev(gamma, dt), _dev(r, dt), SF, NOISE, mode, bad, lm, lv)
    assert int(bad.item()) == (1 if planted else 0)
    mref, vref, h, mumag, lam = sp.loo_rows(a, v, gamma, r, SF, NOISE, mode)
    u = UNIT[dt]
    qd, s, mu = (a * a).sum(axis=1), (v * v).sum(axis=1), v @ gamma
    dlam = (m + 2) * u * qd if mode == 0 else np.zeros(ns)
    dh = (m + 2) * u * s / lam + h * dlam / lam
    bv = dlam / np.abs(1 - h) + lam * dh / (1 - h) ** 2 + 4 * u * np.abs(vref)
    bm = ((m + 2) * u * mumag / np.abs(1 - h)[:, None] + np.abs(r - mu) * (dh / (1 - h) ** 2)[:, None] + 4 * u * np.abs(mref))
    ev = np.abs(lv.double().cpu().numpy() - vref)
    em = np.abs(lm.double().cpu().numpy() - mref)
    print("sparse_loo %s mode %d %s: max err/bound mean %.3e var %.3e" % (dt, mode, (ns, m, q), (em / bm).max(), (ev / bv).max()))
    assert (ev <= bv).all() and (em <= bm).all()
    # either output alone: the same bits; the count accumulates over calls
    l2, v2 = torch.full_like(lm, float("nan")), torch.full_like(lv, float("nan"))
    dev.sparse_loo(ad, vd, ns, m, _dev(gamma, dt), _dev(r, dt), SF, NOISE, mode, bad, l2, None)
    dev.sparse_loo(ad, vd, ns, m, _dev(gamma, dt), _dev(r, dt), SF, NOISE, mode, bad, None, v2)
    assert torch.equal(_bits(l2), _bits(lm)) and torch.equal(_bits(v2), _bits(lv))
    assert int(bad.item()) == (3 if planted else 0)


# ---- cimrgp_sparse_joint_cov -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 3])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_joint_cov_lower_triangle_within_the_componentwise_bound(ca, dt, cov, ns, m, d, q):
    """|err_ij| <= (m + 2) u sum_k (|A A| + |W W|) + u |K| on the lower triangle, whatever the strict upper triangle of C
    holds (NaN here); with a workspace the factor L of the (then positive definite) matrix reproduces it and the strict upper
    triangle is zero."""
    dev = ca.device
    rng = np.random.default_rng(ns + m + d + cov)
    xs = _round(rng.uniform(-2, 2, size=(ns, d)) / np.sqrt(d), dt)
    a, w = _round(rng.normal(size=(ns, m)), dt), _round(rng.normal(size=(ns, m)), dt)
    ld = dev.joint_ld(m, TDT[dt])
    ad, wd, xsd = _padded(ca, a, dt, ld), _padded(ca, w, dt, ld), _dev(xs, dt)
    ldc = dev.joint_ld(ns, TDT[dt])
    c = torch.full((ns, ldc), float("nan"), dtype=TDT[dt], device="cuda")
    dev.sparse_joint_cov(xsd, ELL, SF, 0.25, ad, wd, m, c, cov=cov)
    torch.cuda.synchronize()
    kss = sp.kcov(xs, xs, cov, ELL, SF)
    ref = kss + 0.25 * np.eye(ns) - a @ a.T + w @ w.T
    bound = (m + 2) * UNIT[dt] * (np.abs(a) @ np.abs(a).T + np.abs(w) @ np.abs(w).T) + UNIT[dt] * (np.abs(kss) + 0.25 * np.eye(ns))
    got = c[:, :ns].double().cpu().numpy()
    il, iu = np.tril_indices(ns), np.triu_indices(ns, 1)
    ratio = float((np.abs(got - ref)[il] / bound[il]).max())
    print("sparse_joint_cov %s cov %d %s: max err/bound %.3e" % (dt, cov, (ns, m, d), ratio))
    assert ratio <= 1.0
    assert bool(torch.isnan(c[:, ns:]).all())            # (the Gram's diagonal tiles may write above the diagonal)
    # factored: A* small, W* of unit scale and 1.0 on the diagonal make it positive definite
    a2 = _round(a * 0.1 / np.sqrt(m), dt)
    ad2 = _padded(ca, a2, dt, ld)
    ref2 = kss + np.eye(ns) - a2 @ a2.T + w @ w.T
    ws = dev.potrf_workspace(ns, TDT[dt], "cuda")
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    c.fill_(float("nan"))
    dev.sparse_joint_cov(xsd, ELL, SF, 1.0, ad2, wd, m, c, ws, info, cov=cov)
    assert int(info.item()) == 0
    low = c[:, :ns].double().cpu().numpy()
    assert (low[iu] == 0).all() and np.isfinite(low).all()
    # Higham, Accuracy and Stability, thm 10.3: |C - L L^T| <= (ns + 1) u |L| |L^T| <= (ns + 1) u max diag, beside the
    # bound of the matrix that was factored
    tol = (ns + 1) * UNIT[dt] * np.diag(ref2).max() * 2 + ((m + 2) * UNIT[dt] * (np.abs(a2) @ np.abs(a2).T + np.abs(w) @ np.abs(w).T)
                                                          + UNIT[dt] * (np.abs(kss) + np.eye(ns))).max()
    assert np.abs(low @ low.T - ref2).max() <= tol


# ---- SparseBlock: predict_grad, loo, joint against the oracle ----------------------------------------------------------
N, M = 1500, 150
_CASES = {}


def _kernel(ca, cov, ell, noise=NOISE):
    if cov == 0:
        return ca.RBFKernel(l=ell, sf=SF, noise=noise)
    return ca.DenseMaternKernel(nu={1: 0.5, 2: 1.5, 3: 2.5}[cov], l=ell, sf=SF, noise=noise)


def _case(ca, d, cov, mode):
    """One fitted block and its oracle (Woodbury and dense), shared by the three tests; one case is kept at a time."""
    key = (d, cov, mode)
    if key not in _CASES:
        _CASES.clear()
        from cimrgp_amd.Sparse import SparseBlock
        x, z, r, xs = sp.problem(N, M, d, seed=N + M + d + cov, q=2)
        fit = sp.Fit(x, z, r, cov, ELL, SF, NOISE, EPS, mode)
        blk = SparseBlock(_dev(x, "f64"), _dev(z, "f64"), _kernel(ca, cov, ELL), 'fitc' if mode == 0 else 'vfe', EPS)
        blk.fit(_dev(r, "f64"))
        _CASES[key] = (fit, xs, blk, _dev(xs, "f64"), _dev(r, "f64"))
    return _CASES[key]


def _tol(*gaps):
    """100 x the oracle's own Woodbury-against-dense gap on the same inputs, floor 1e-9 (relative)."""
    return max(1e-9, 100.0 * max(gaps))


CASES = [(d, cov, mode) for d in (1, 2, 3) for cov in (0, 1, 2, 3) for mode in (0, 1)]


@pytest.mark.parametrize("d,cov,mode", CASES)
def test_block_predict_grad_matches_the_oracle(ca, d, cov, mode):
    fit, xs, blk, xsd, _ = _case(ca, d, cov, mode)
    mg = torch.full((xs.shape[0], d, 2), float("nan"), dtype=torch.float64, device="cuda")
    vg = torch.full((xs.shape[0], d), float("nan"), dtype=torch.float64, device="cuda")
    blk.predict_grad(xsd, mg, vg)
    wm, wv = sp.predict_grad(fit, xs)
    dm, dv = sp.predict_grad_dense(fit, xs)
    tol = _tol(sp.rel(wm, dm), sp.rel(wv, dv))
    gm, gv = sp.rel(mg.cpu().numpy(), wm), sp.rel(vg.cpu().numpy(), wv)
    print("predict_grad d %d cov %d mode %d: mean %.2e var %.2e tolerance %.2e" % (d, cov, mode, gm, gv, tol))
    assert gm <= tol and gv <= tol
    # either output alone: the same bits
    m2, v2 = torch.empty_like(mg), torch.empty_like(vg)
    blk.predict_grad(xsd, m2, None)
    blk.predict_grad(xsd, None, v2)
    assert torch.equal(_bits(m2), _bits(mg)) and torch.equal(_bits(v2), _bits(vg))


@pytest.mark.parametrize("d,cov,mode", CASES)
def test_block_loo_matches_the_oracle_on_every_row(ca, d, cov, mode):
    fit, xs, blk, _, rd = _case(ca, d, cov, mode)
    lm, lv, h = sp.loo(fit)
    assert h.max() < 0.99
    dm, dv = sp.loo_dense(fit)
    tol = _tol(sp.rel(lm, dm), sp.rel(lv, dv))
    mean, var = torch.empty_like(rd), torch.empty(N, dtype=torch.float64, device="cuda")
    blk.loo(rd, mean, var)
    gm, gv = sp.rel(mean.cpu().numpy(), lm), sp.rel(var.cpu().numpy(), lv)
    print("loo d %d cov %d mode %d: mean %.2e var %.2e tolerance %.2e max h %.3f" % (d, cov, mode, gm, gv, tol, h.max()))
    assert gm <= tol and gv <= tol


@pytest.mark.parametrize("d,cov,mode", CASES)
def test_block_joint_covariance_matches_the_oracle(ca, d, cov, mode):
    fit, xs, blk, xsd, _ = _case(ca, d, cov, mode)
    ns = xs.shape[0]
    c, _, _ = sp.joint_cov(fit, xs)
    tol = _tol(sp.rel(c, sp.joint_cov_dense(fit, xs)))
    out = torch.zeros((ns, ns), dtype=torch.float64, device="cuda")
    assert blk.joint(xsd, cov_out=out) == 0.0
    got = out.cpu().numpy()
    assert (got[np.triu_indices(ns, 1)] == 0).all()
    gap = sp.rel(np.tril(got), np.tril(c))
    print("joint d %d cov %d mode %d: %.2e tolerance %.2e" % (d, cov, mode, gap, tol))
    assert gap <= tol
    # its diagonal is predict's variance; include_noise adds the noise to the diagonal alone
    var = torch.empty(ns, dtype=torch.float64, device="cuda")
    blk.predict(xsd, None, var)
    assert sp.rel(np.diag(got), var.cpu().numpy()) <= 1e-12
    noisy = torch.zeros((ns, ns), dtype=torch.float64, device="cuda")
    blk.joint(xsd, cov_out=noisy, include_noise=True)
    assert np.abs(noisy.cpu().numpy() - got - NOISE * np.eye(ns)).max() <= 1e-14


@pytest.mark.parametrize("mode", [0, 1])
def test_block_with_lengthscales_matches_the_oracle_on_scaled_inputs(ca, mode):
    """ARD (0.7, 1.3): the block on x with lengthscales equals the oracle at l = 1 on x / l; gradients come back in the
    caller's units (the oracle's divided by l_e)."""
    from cimrgp_amd.Sparse import SparseBlock
    d, cov, ls = 2, 0, np.array([0.7, 1.3])
    x, z, r, xs = sp.problem(N, M, d, seed=N + M + d, q=2)
    fit = sp.Fit(x / ls, z / ls, r, cov, 1.0, SF, NOISE, EPS, mode)
    blk = SparseBlock(_dev(x, "f64"), _dev(z, "f64"), _kernel(ca, cov, 1.0), 'fitc' if mode == 0 else 'vfe', EPS, lengthscales=ls)
    rd, xsd = _dev(r, "f64"), _dev(xs, "f64")
    blk.fit(rd)
    ns = xs.shape[0]
    mg = torch.empty((ns, d, 2), dtype=torch.float64, device="cuda")
    vg = torch.empty((ns, d), dtype=torch.float64, device="cuda")
    blk.predict_grad(xsd, mg, vg)
    wm, wv = sp.predict_grad(fit, xs / ls)
    dm, dv = sp.predict_grad_dense(fit, xs / ls)
    tol = _tol(sp.rel(wm, dm), sp.rel(wv, dv))
    assert sp.rel(mg.cpu().numpy(), wm / ls[None, :, None]) <= tol and sp.rel(vg.cpu().numpy(), wv / ls[None, :]) <= tol
    lm, lv, h = sp.loo(fit)
    dlm, dlv = sp.loo_dense(fit)
    mean, var = torch.empty_like(rd), torch.empty(N, dtype=torch.float64, device="cuda")
    blk.loo(rd, mean, var)
    tol = _tol(sp.rel(lm, dlm), sp.rel(lv, dlv))
    assert h.max() < 0.99 and sp.rel(mean.cpu().numpy(), lm) <= tol and sp.rel(var.cpu().numpy(), lv) <= tol
    c, _, _ = sp.joint_cov(fit, xs / ls)
    out = torch.zeros((ns, ns), dtype=torch.float64, device="cuda")
    blk.joint(xsd, cov_out=out)
    assert sp.rel(np.tril(out.cpu().numpy()), np.tril(c)) <= _tol(sp.rel(c, sp.joint_cov_dense(fit, xs / ls)))


# ---- the plugins ---------------------------------------------------------------------------------------------------------
def _raw(n, d, seed, ns=257):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d)) * np.arange(1, d + 1) + 3.0
    y = np.stack([np.sin(2 * x).sum(axis=1), np.cos(x).prod(axis=1)], axis=1) * 2.0 + 0.5 + 0.1 * rng.normal(size=(n, 2))
    xs = rng.uniform(-2.2, 2.2, size=(ns, d)) * np.arange(1, d + 1) + 3.0
    return x, y, xs


def _plugin(ca, mode, m, cov, ell, **kw):
    cls = ca.SGP_FITC if mode == 0 else ca.SparseGP_RBF
    return cls(num_inducing=m, lengthscale=ell, variance=SF, nu={0: None, 1: 0.5, 2: 1.5, 3: 2.5}[cov], **kw)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [2, 3])
def test_plugin_gradients_match_central_differences_of_its_own_prediction(ca, d, cov, mode):
    """predictive_gradients against central differences (h = 1e-5 in z-scored input units) of predict_with_variance, at the
    host test's bar; the covariance's diagonal is that variance."""
    x, y, xs = _raw(N, d, 10 + d + cov)
    g = _plugin(ca, mode, M, cov, ELL)
    g.fit([x, y])
    dmu, dvar = g.predictive_gradients(xs)
    assert dmu.shape == (257, d, 2) and dvar.shape == (257, d)
    sd = x.std(axis=0)
    cm, cv = np.zeros_like(dmu), np.zeros_like(dvar)
    for e in range(d):
        step = np.zeros(d)
        step[e] = 1e-5 * sd[e]
        mp, vp = g.predict_with_variance(xs + step)
        mm, vm = g.predict_with_variance(xs - step)
        cm[:, e, :], cv[:, e] = (mp - mm) / (2 * step[e]), (vp - vm) / (2 * step[e])
    gm, gv = sp.rel(cm, dmu), sp.rel(cv, dvar)
    print("plugin gradients d %d cov %d mode %d: mean %.2e var %.2e bar %.2e" % (d, cov, mode, gm, gv, MARGIN * CENTRAL_LEVEL))
    assert gm <= MARGIN * CENTRAL_LEVEL and gv <= MARGIN * CENTRAL_LEVEL
    mean, var = g.predict_with_variance(xs)
    mean_c, cov_c = g.predict_with_covariance(xs)
    assert np.array_equal(mean_c, mean) and np.array_equal(cov_c, cov_c.T)
    assert sp.rel(np.diag(cov_c), var) <= 1e-12


@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_gradients_and_loo_are_bit_equal(ca, mode):
    x, y, xs = _raw(N, 2, 3, ns=600)
    g = _plugin(ca, mode, M, 2, ELL)
    g.fit([x, y])
    assert g.block.grad_chunk_rows(1) == 256 and g.block.grad_chunk_rows() > 600 and g.block.chunk_rows(1) == 256
    dmu, dvar = g.predictive_gradients(xs)
    dmu_c, dvar_c = g.predictive_gradients(xs, budget_bytes=1)          # 256 rows at a time: 3 chunks
    assert np.array_equal(dmu, dmu_c) and np.array_equal(dvar, dvar_c)
    mean, var = g.leave_one_out()
    mean_c, var_c = g.leave_one_out(budget_bytes=1)                     # 6 chunks
    assert np.array_equal(mean, mean_c) and np.array_equal(var, var_c)
    lpd = g.loo_log_predictive_density()
    yz, mz = (y - y.mean(axis=0)) / y.std(axis=0), (mean - y.mean(axis=0)) / y.std(axis=0)
    assert sp.rel(lpd, -0.5 * 2 * np.log(2 * np.pi * var) - 0.5 * ((yz - mz) ** 2).sum(axis=1) / var) <= 1e-10
    assert lpd.shape == (N,) and np.isfinite(lpd).all()


def test_samples_prefix_seed_and_moments(ca):
    x, y, _ = _raw(N, 2, 5)
    xs = np.random.default_rng(6).uniform(-2.2, 2.2, size=(32, 2)) * np.arange(1, 3) + 3.0
    g = _plugin(ca, 0, M, 0, ELL)
    g.fit([x, y])
    s20 = g.posterior_samples_f(xs, size=20, seed=3)
    s5 = g.posterior_samples_f(xs, size=5, seed=3)
    assert s20.shape == (20, 32, 2) and np.array_equal(s5, s20[:5])
    assert np.array_equal(g.posterior_samples_f(xs, size=5, seed=3), s5)
    assert not np.array_equal(g.posterior_samples_f(xs, size=5, seed=4), s5)
    draws = 4096
    s = g.posterior_samples_f(xs, size=draws, seed=11)
    mean, cov = g.predict_with_covariance(xs)
    ys = y.std(axis=0)
    sig = cov + 1e-6 * SF * np.eye(32)                                   # what the draws are made with
    for c in range(2):
        z = (s[:, :, c] - mean[None, :, c]) / ys[c]
        se_mean = np.sqrt(np.diag(sig) / draws)
        assert (np.abs(z.mean(axis=0)) <= 5 * se_mean).all()
        emp = z.T @ z / draws
        se_cov = np.sqrt((sig ** 2 + np.outer(np.diag(sig), np.diag(sig))) / draws)
        assert (np.abs(emp - sig) <= 5 * se_cov).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [1, 2])
def test_inducing_at_the_data_gives_the_exact_plugins_loo_and_gradients(ca, d, mode):
    """Z = X, eps = 0, Matern 1/2: leave_one_out and predictive_gradients of GP_Matern(0.5, optimize=False) at the same
    length-scale and variance, to 1e-9."""
    x, y, xs = _raw(600, d, 40 + d)
    g = _plugin(ca, mode, 600, 1, 1.0, Z=x, jitter=0.0)
    g.fit([x, y])
    e = ca.GP_Matern(0.5, 1.0, SF, optimize=False)
    e.fit([x, y])
    (lm, lv), (em, ev) = g.leave_one_out(), e.leave_one_out()
    (gm, gv), (xm, xv) = g.predictive_gradients(xs), e.predictive_gradients(xs)
    print("Z = X d=%d mode %d: loo %.2e %.2e grad %.2e %.2e" % (d, mode, sp.rel(lm, em), sp.rel(lv, ev), sp.rel(gm, xm), sp.rel(gv, xv)))
    assert sp.rel(lm, em) <= 1e-9 and sp.rel(lv, ev) <= 1e-9
    assert sp.rel(gm, xm) <= 1e-9 and sp.rel(gv, xv) <= 1e-9
