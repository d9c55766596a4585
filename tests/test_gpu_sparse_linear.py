"""GPU tests of the sparse GP's linear term (include/cimrgp_sparse_linear.h; DESIGN.md, "A linear term for the sparse GP").
Kernel level: the four entry points against extended-precision NumPy at their componentwise bounds and against their twins
bit for bit.  Block level: SparseBlock(linear=) against the oracle of tests/sparse_linear_numpy.py.  Plugin:
SparseGP_RBFLinear through the z-scoring, its gradient against central differences, the optimisers, and the extrapolation of
a trend."""
import numpy as np
import pytest

import sparse_ard_numpy as sa
import sparse_linear_numpy as sl
import sparse_numpy as sn
from test_sparse_linear_host import CENTRAL_LEVEL, MARGIN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
#: (na, nb, d): one row; one tile, ragged; four row tiles; 3 column tiles x 3 row slices of the pair contraction; the largest d
SHAPES = [(1, 16, 1), (65, 63, 2), (255, 100, 2), (600, 257, 3), (257, 1000, 8)]
ELL, SF = 0.7, 1.3
#: roundings k_cov may be off its extended-precision value: 10 x the 35.9 that FP64 NumPy spends on the same expression
#: against numpy.longdouble over these shapes and the four covariances (measured once, on the host; the rule of
#: tests/test_gpu_sparse_post.py)
K_ROUNDINGS = 360.0
#: powers of two: lin[e] xb_je is then exact in both dtypes, and the term costs exactly d roundings for the dot product and one
#: for its sum with k_cov
LIN8 = np.array([0.5, 0.25, 2.0, 0.125, 1.0, 0.5, 0.25, 4.0])
#: weights of no special form, for the contraction (its sums are FP64)
LINR = np.array([0.5, 0.2, 0.35, 0.11, 0.7, 0.05, 0.9, 0.41])


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


def _f64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


def _points(na, nb, d, dt, seed):
    rng = np.random.default_rng(seed)
    xb = _round(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d), dt)
    xa = _round(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d), dt)
    k = min(na, nb) // 2 + 1
    xa[:k] = xb[:k]                                      # pairs at r = 0
    return xa, xb


def _lin_terms(xa, xb, lin):
    """(sum_e lin_e xa_e xb_e, sum_e |.|) in extended precision."""
    t = np.asarray(xa, dtype=np.longdouble)[:, None, :] * np.asarray(xb, dtype=np.longdouble)[None, :, :] * np.asarray(lin, np.longdouble)
    return t.sum(-1), np.abs(t).sum(-1)


# ---- cimrgp_cov_cross_lin / cimrgp_cov_gram_lin -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("na,nb,d", SHAPES)
def test_cov_cross_lin_within_roundings_and_its_twin_at_zero(ca, dt, cov, na, nb, d):
    """|err| <= K_ROUNDINGS u |k_cov| + (d + 1) u (|k_cov| + sum_e |lin_e xa_e xb_e|): the twin's rule, and d + 1 more roundings
    (d of the dot product's multiply-adds, one of its sum with k_cov), each of at most u times the magnitude of what is summed."""
    dev, devl = ca.device, ca.device_linear
    xa, xb = _points(na, nb, d, dt, na + nb + d + cov)
    xad, xbd = _dev(xa, dt), _dev(xb, dt)
    lin = LIN8[:d]
    out = dev.alloc_matrix(na, nb, TDT[dt], "cuda")
    out.fill_(float("nan"))
    devl.cov_cross_lin(xad, xbd, ELL, SF, _f64(lin), out=out, cov=cov)
    twin = dev.rbf_cross(xad, xbd, ELL, SF, cov=cov)
    zero = devl.cov_cross_lin(xad, xbd, ELL, SF, _f64(np.zeros(d)), cov=cov)
    torch.cuda.synchronize()
    assert torch.equal(_bits(zero[:na, :nb]), _bits(twin[:na, :nb]))
    assert bool(torch.isnan(out[:, nb:]).all())          # padding columns are not written
    kl, _, _ = sa.k_and_g(xa, xb, cov, ELL, SF, np.longdouble)
    dot, mag = _lin_terms(xa, xb, lin)
    ref = np.asarray(kl + dot, dtype=np.float64)
    got = out[:na, :nb].double().cpu().numpy()
    bound = UNIT[dt] * (K_ROUNDINGS * np.abs(kl) + (d + 1) * (np.abs(kl) + mag)).astype(np.float64)
    worst = float((np.abs(got - ref) / bound).max())
    print("cov_cross_lin %s cov %d %s: max err/bound %.3e" % (dt, cov, (na, nb, d), worst))
    assert np.isfinite(got).all() and worst <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("na,nb,d", SHAPES)
def test_cov_gram_lin_within_roundings_diag_add_on_the_diagonal_only(ca, dt, cov, na, nb, d):
    dev, devl = ca.device, ca.device_linear
    _, x = _points(na, nb, d, dt, na + nb + d + cov)
    n = nb
    xd = _dev(x, dt)
    lin = LIN8[:d]
    diag = 0.375
    full = dev.alloc_matrix(n, n, TDT[dt], "cuda")
    full.fill_(float("nan"))
    devl.cov_gram_lin(xd, ELL, SF, _f64(lin), diag, out=full, cov=cov)
    low = dev.alloc_matrix(n, n, TDT[dt], "cuda")
    low.fill_(float("nan"))
    devl.cov_gram_lin(xd, ELL, SF, _f64(lin), diag, lower_only=True, out=low, cov=cov)
    plain = devl.cov_gram_lin(xd, ELL, SF, _f64(lin), 0.0, cov=cov)
    cross = devl.cov_cross_lin(xd, xd, ELL, SF, _f64(lin), cov=cov)
    zero = devl.cov_gram_lin(xd, ELL, SF, _f64(np.zeros(d)), diag, cov=cov)
    twin = dev.rbf_gram(xd, ELL, SF, diag, cov=cov)      # all tiles: the 64 x 64 kernel
    torch.cuda.synchronize()
    assert torch.equal(_bits(zero[:n, :n]), _bits(twin[:n, :n]))
    assert torch.equal(_bits(plain[:n, :n]), _bits(cross[:n, :n]))
    # diag_add: the diagonal only, added to the rounded element in the dtype
    f, p = full[:n, :n], plain[:n, :n]
    off = ~torch.eye(n, dtype=torch.bool, device="cuda")
    assert torch.equal(_bits(f[off]), _bits(p[off]))
    assert torch.equal(_bits(torch.diagonal(f)), _bits(torch.diagonal(p) + torch.tensor(diag, dtype=TDT[dt], device="cuda")))
    # the lower triangle alone: the same bits at j <= i; whole tiles above the diagonal tiles are not written
    tri = torch.tril(torch.ones(n, n, dtype=torch.bool, device="cuda"))
    assert torch.equal(_bits(low[:n, :n][tri]), _bits(f[tri]))
    if n > 64:
        assert bool(torch.isnan(low[:64, 64:n]).all())
    assert bool(torch.isnan(full[:, n:]).all()) and bool(torch.isnan(low[:, n:]).all())
    kl, _, _ = sa.k_and_g(x, x, cov, ELL, SF, np.longdouble)
    dot, mag = _lin_terms(x, x, lin)
    ref = np.asarray(kl + dot, dtype=np.float64)
    got = p.double().cpu().numpy()
    bound = UNIT[dt] * (K_ROUNDINGS * np.abs(kl) + (d + 1) * (np.abs(kl) + mag)).astype(np.float64)
    worst = float((np.abs(got - ref) / bound).max())
    print("cov_gram_lin %s cov %d %s: max err/bound %.3e" % (dt, cov, (n, d), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cov_cross_lin_odd_pitch_and_offset_view(ca, dt):
    """An output whose pitch is no multiple of 16 bytes, at an offset: the element-wise store path writes the same bits as the
    16-byte stores, and nothing beside them."""
    dev, devl = ca.device, ca.device_linear
    na, nb, d = 255, 100, 2
    xa, xb = _points(na, nb, d, dt, 5)
    xad, xbd, lin = _dev(xa, dt), _dev(xb, dt), _f64(LIN8[:d])
    want = devl.cov_cross_lin(xad, xbd, ELL, SF, lin, cov=2)
    big = torch.full((na + 2, nb + 7), float("nan"), dtype=TDT[dt], device="cuda")       # pitch 107 elements
    view = big[1:na + 1, 3:nb + 3]
    assert (view.stride(0) * view.element_size()) % 16 != 0
    devl.cov_cross_lin(xad, xbd, ELL, SF, lin, out=view, cov=2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(view), _bits(want[:na, :nb]))
    big[1:na + 1, 3:nb + 3] = 0
    assert int(torch.isnan(big).sum()) == big.numel() - na * nb
    # the inputs as views at an offset too
    xbig = torch.zeros((na + 3, d), dtype=TDT[dt], device="cuda")
    xbig[2:na + 2] = xad
    again = devl.cov_cross_lin(xbig[2:na + 2], xbd, ELL, SF, lin, cov=2)
    assert torch.equal(_bits(again[:na, :nb]), _bits(want[:na, :nb]))


# ---- cimrgp_sparse_lambda_kd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 16), (255, 100), (600, 257), (1500, 1000)])
def test_sparse_lambda_kd_is_its_twin_at_a_constant_diagonal_and_numpy_at_a_varying_one(ca, dt, mode, n, m):
    dev, devl, tdt = ca.device, ca.device_linear, TDT[dt]
    rng = np.random.default_rng(n + m)
    a = _round(rng.normal(size=(n, m)) * 0.5 / np.sqrt(m), dt)
    sf2, noise = 1.25, 0.02                               # sf2: a value of both dtypes
    abuf = dev.alloc_matrix(n, m, tdt, "cuda")
    abuf.fill_(float("nan"))
    abuf[:n, :m] = _dev(a, dt)
    lam0, w0, s0 = dev.sparse_lambda(abuf, n, m, sf2, noise, mode)
    lam1, w1, s1 = devl.sparse_lambda_kd(abuf, n, m, torch.full((n,), sf2, dtype=tdt, device="cuda"), noise, mode)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lam0), _bits(lam1)) and torch.equal(_bits(w0), _bits(w1)) and torch.equal(_bits(s0), _bits(s1))
    # a varying diagonal, one row with k_ii too small for a positive lambda: the twin's bounds
    kd = _round(sf2 + rng.uniform(0.0, 2.0, size=n), dt)
    if n > 4:
        kd[3] = _round(-0.5, dt)
    lam, w, sums = devl.sparse_lambda_kd(abuf, n, m, _dev(kd, dt), noise, mode)
    qd = (a * a).sum(axis=1)
    lam_ref = kd - qd + noise if mode == 0 else np.full(n, noise)
    tol = 1e-14 if dt == "f64" else 1e-6
    lam_h, w_h, s = lam.double().cpu().numpy(), w.double().cpu().numpy(), sums.cpu().numpy()
    assert np.abs(lam_h - lam_ref).max() <= tol * (np.abs(kd).max() + noise + qd.max())
    assert np.abs(w_h * lam_h - 1).max() <= 4 * UNIT[dt]
    bad = int((lam_ref <= 0).sum())
    assert int(s[2]) == bad and bad == (1 if (mode == 0 and n > 4) else 0)
    if bad == 0:
        assert abs(s[0] - np.log(lam_h).sum()) <= 1e-13 * np.abs(np.log(lam_h)).sum()
    d_ref = _round(kd - qd, dt)
    assert abs(s[1] - d_ref.sum()) <= (1e-13 if dt == "f64" else 1e-6) * np.abs(d_ref).sum()


# ---- cimrgp_cov_pair_grad_lin ----------------------------------------------------------------------------------------
def _pair_case(ca, dt, cov, na, nb, d):
    dev = ca.device
    xa, xb = _points(na, nb, d, dt, na + nb + d + cov)
    rng = np.random.default_rng(7 * na + nb)
    g = _round(rng.normal(size=(na, nb)), dt)
    gbuf = dev.alloc_matrix(na, nb, TDT[dt], "cuda")
    gbuf.fill_(float("nan"))
    gbuf[:na, :nb] = _dev(g, dt)
    return xa, xb, g, _dev(xa, dt), _dev(xb, dt), gbuf


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("na,nb,d", SHAPES)
def test_cov_pair_grad_lin_against_its_twins_and_numpy(ca, dt, cov, na, nb, d):
    """sums are the twin's bits with and without weights; at lin = 0 so is db.  lsums and the linear share of db (the run with
    weights minus the run without, in FP64) are FP64 sums of na (and nb) terms: |err| <= (na + 2) u64 sum |terms|, plus, for
    db, the roundings that end each of the two runs (the sum of the two shares, the scale, the dtype): 2 u_dtype |db| each."""
    dev, devl = ca.device, ca.device_linear
    xa, xb, g, xad, xbd, gbuf = _pair_case(ca, dt, cov, na, nb, d)
    lin = LINR[:d]
    u64 = UNIT["f64"]
    for ard, twin in ((False, dev.cov_pair_grad), (True, dev.cov_pair_grad_ard)):
        ts, tdb = twin(xad, xbd, gbuf, ELL, SF, scale=1.5, cov=cov)
        zs, zl, zdb = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, _f64(np.zeros(d)), ard=ard, scale=1.5, cov=cov)
        s, ls, db = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, _f64(lin), ard=ard, scale=1.5, cov=cov)
        s2, ls2, db2 = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, _f64(lin), ard=ard, scale=1.5, cov=cov)
        torch.cuda.synchronize()
        assert torch.equal(_bits(zs), _bits(ts)) and torch.equal(_bits(zdb), _bits(tdb))
        assert torch.equal(_bits(s), _bits(ts))
        assert torch.equal(_bits(ls), _bits(zl))         # lsums does not depend on the weights
        assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_bits(ls), _bits(ls2)) and torch.equal(_bits(db), _bits(db2))
        (_, lref, _, dblin), (_, lmag, dbmag) = sl.pair_grad_lin(xa, xb, g, cov, ELL, SF, lin, ard, 1.5, np.longdouble)
        rl = float((np.abs(ls.cpu().numpy() - lref) / ((na + 2) * u64 * lmag)).max())
        dbh, zdbh = db.double().cpu().numpy(), zdb.double().cpu().numpy()
        bound = (na + 2) * u64 * dbmag + 2 * UNIT[dt] * (np.abs(dbh) + np.abs(zdbh))
        rd = float((np.abs((dbh - zdbh) - dblin) / bound).max())
        print("cov_pair_grad_lin %s cov %d ard %d %s: max err/bound lsums %.3e db %.3e" % (dt, cov, ard, (na, nb, d), rl, rd))
        assert rl <= 1.0 and rd <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ard", [False, True])
def test_cov_pair_grad_lin_accumulate_scale_and_null_outputs(ca, dt, ard):
    """accumulate adds to all three outputs; scale multiplies the db sum only, the linear share included; an output that is
    NULL is left out and the others keep their bits; all three NULL: nothing is done."""
    dev, devl = ca.device, ca.device_linear
    na, nb, d, cov = 600, 257, 3, 2
    xa, xb, g, xad, xbd, gbuf = _pair_case(ca, dt, cov, na, nb, d)
    lin = _f64(LINR[:d])
    s, ls, db = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, cov=cov)
    s1, ls1, db1 = s.clone(), ls.clone(), db.clone()
    devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, scale=2.0, accumulate=True, sums=s1, lsums=ls1, db=db1, cov=cov)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1), _bits(s + s)) and torch.equal(_bits(ls1), _bits(ls + ls))
    if dt == "f64":
        assert torch.equal(_bits(db1), _bits(db + 2.0 * db))
    else:                                                # (float)((double)(float)x + 2 x): within two roundings of 3 (float)x
        assert bool(((db1 - 3.0 * db).abs() <= 4 * UNIT[dt] * (3.0 * db).abs()).all())
    # scale alone
    _, _, dbs = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, scale=-4.0, cov=cov, want_sums=False, want_lsums=False)
    assert torch.equal(_bits(dbs), _bits(-4.0 * db))
    # NULL combinations
    only_s, none_l, none_db = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, cov=cov, want_lsums=False, want_db=False)
    assert none_l is None and none_db is None and torch.equal(_bits(only_s), _bits(s))
    none_s, only_l, none_db = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, cov=cov, want_sums=False, want_db=False)
    assert none_s is None and none_db is None and torch.equal(_bits(only_l), _bits(ls))
    none_s, none_l, only_db = devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, cov=cov, want_sums=False, want_lsums=False)
    assert none_s is None and none_l is None and torch.equal(_bits(only_db), _bits(db))
    scratch = torch.full((devl.cov_pair_grad_lin_scratch_bytes(na, nb, d, ard),), 0x5A, dtype=torch.uint8, device="cuda")
    devl.cov_pair_grad_lin(xad, xbd, gbuf, ELL, SF, lin, ard=ard, cov=cov, want_sums=False, want_lsums=False, want_db=False,
                           scratch=scratch)
    torch.cuda.synchronize()
    assert bool((scratch == 0x5A).all())


# ---- SparseBlock(linear=) --------------------------------------------------------------------------------------------
N, M, NS, Q, NOISE, EPS = 1500, 150, 257, 2, 0.02, 1e-6
ARD_ELLS = (0.7, 1.3)
V = (0.5, 0.2, 0.35)
_ORACLE = {}


def _block_case(d, cov, mode, ard):
    """The oracle's numbers of one block case, computed once and shared: inputs, both forms, the gradient."""
    key = (d, cov, mode, ard)
    if key not in _ORACLE:
        x, z, r, xs = sn.problem(N, M, d, 40 + d)
        z = z + 0.05 * np.random.default_rng(41).normal(size=z.shape)
        ell = np.array([ARD_ELLS[e % 2] for e in range(d)]) if ard else 0.9
        lin = np.array(V[:d])
        args = (x, z, r, cov, ell, SF, NOISE, EPS, mode, lin)
        wood = [sl.woodbury(*args, xs, noise) for noise in (False, True)]
        dens = [sl.dense(*args, xs, noise) for noise in (False, True)]
        _ORACLE[key] = dict(x=x, z=z, r=r, xs=xs, ell=ell, lin=lin, wood=wood, dens=dens, grad=sl.grad_dense(*args),
                            grad_wood=sl.grad_woodbury(*args))
    return _ORACLE[key]


def _gap(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _make_block(ca, c, cov, mode, ard, linear=True):
    from cimrgp_amd.Sparse import SparseBlock
    nu = {0: None, 1: 0.5, 2: 1.5, 3: 2.5}[cov]
    ell = 1.0 if ard else float(c["ell"])
    kern = ca.RBFKernel(l=ell, sf=SF, noise=NOISE) if nu is None else ca.DenseMaternKernel(nu=nu, l=ell, sf=SF, noise=NOISE)
    kw = dict(lengthscales=c["ell"]) if ard else {}
    if linear:
        kw["linear"] = c["lin"]
    return SparseBlock(_dev(c["x"], "f64"), _dev(c["z"], "f64"), kern, ("fitc", "vfe")[mode], EPS, **kw)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_block_fit_predict_and_objective_against_the_oracle(ca, d, cov, mode, ard):
    """Bound: 100 x the oracle's own Woodbury-vs-dense gap on the same inputs, floor 1e-9 relative."""
    c = _block_case(d, cov, mode, ard)
    blk = _make_block(ca, c, cov, mode, ard).fit(_dev(c["r"], "f64"))
    lml = blk.log_marginal_likelihood()
    xs = _dev(c["xs"], "f64")
    for k, include_noise in enumerate((False, True)):
        (wl, wm, wv), (dl, dm, dv) = c["wood"][k], c["dens"][k]
        mean = torch.full((NS, Q), float("nan"), dtype=torch.float64, device="cuda")
        var = torch.full((NS,), float("nan"), dtype=torch.float64, device="cuda")
        blk.predict(xs, mean, var, include_noise=include_noise, budget_bytes=1 << 19)     # several chunks
        tol_l = max(100 * abs(wl - dl) / abs(dl), 1e-9)
        tol_m, tol_v = max(100 * _gap(wm, dm), 1e-9), max(100 * _gap(wv, dv), 1e-9)
        gm, gv = _gap(mean.cpu().numpy(), wm), _gap(var.cpu().numpy(), wv)
        print("block d %d cov %d mode %d ard %d noise %d: lml %.2e (tol %.2e) mean %.2e (%.2e) var %.2e (%.2e)"
              % (d, cov, mode, ard, include_noise, abs(lml - wl) / abs(wl), tol_l, gm, tol_m, gv, tol_v))
        assert abs(lml - wl) <= tol_l * abs(wl) and gm <= tol_m and gv <= tol_v
    # the mean alone and the variance alone: the same bits
    m2 = torch.empty_like(mean)
    v2 = torch.empty_like(var)
    blk.predict(xs, m2, None, budget_bytes=1 << 19)
    blk.predict(xs, None, v2, include_noise=True, budget_bytes=1 << 19)
    assert torch.equal(_bits(m2), _bits(mean)) and torch.equal(_bits(v2), _bits(var))


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_block_lml_grad_against_the_oracle(ca, d, cov, mode, ard):
    """Against the gradient from the dense definition.  Bound: the rule of the fit and the prediction above and of
    tests/test_gpu_sparse_grad.py: 100 x the oracle's own gap on the same inputs -- here between its two gradient forms,
    autograd of the dense definition and of the Woodbury chain -- floor 1e-9, per vector relative to its largest entry.
    Where the oracle is good to 1e-11 that is 1e-9, far below 10 x the central-difference figure (4.8e-6); with the RBF at
    d = 1, where m = 150 inducing inputs on a line make cond(K_uu + eps sf I) 1e8, the oracle's own two forms differ by up
    to 2.6e-6 in dZ and the bound is 100 x that.  Measured on the device there (FITC, isotropic): theta 1.5e-13, dZ 2.6e-5.
    The identity 1/2 tr M = sum G o K holds to 1e-9 and the LML is log_marginal_likelihood()'s bit for bit."""
    c = _block_case(d, cov, mode, ard)
    olml, odth, odz = c["grad"]
    _, wdth, wdz = c["grad_wood"]
    tol_t, tol_z = max(100 * _gap(wdth, odth), 1e-9), max(100 * _gap(wdz, odz), 1e-9)
    r = _dev(c["r"], "f64")
    blk = _make_block(ca, c, cov, mode, ard)
    lml, dth, dz = blk.lml_grad(r)
    assert dth.shape == odth.shape == (2 + np.size(c["ell"]) + d,)
    gt, gz = _gap(dth, odth), _gap(dz.cpu().numpy(), odz)
    chk = blk.grad_check
    ident = abs(chk["closed"] - chk["pairwise"]) / abs(chk["closed"])
    print("lml_grad d %d cov %d mode %d ard %d: theta %.2e (bound %.2e) dZ %.2e (bound %.2e) identity %.2e"
          % (d, cov, mode, ard, gt, tol_t, gz, tol_z, ident))
    assert gt <= tol_t and gz <= tol_z
    assert ident <= 1e-9
    assert lml == blk.log_marginal_likelihood() == _make_block(ca, c, cov, mode, ard).fit(r).log_marginal_likelihood()
    assert abs(lml - olml) <= 1e-9 * abs(olml) + 100 * abs(c["wood"][0][0] - c["dens"][0][0])
    lml2, dth2, none = _make_block(ca, c, cov, mode, ard).lml_grad(r, want_z=False)
    assert none is None and lml2 == lml and np.array_equal(dth2, dth)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_block_without_the_term_is_untouched_by_a_linear_block_beside_it(ca, mode, ard):
    """linear=None takes the calls it took before the term existed: its results are the bits of the same block fitted before
    and after a linear block ran on the same data, and of its calls made by hand through the twins."""
    dev = ca.device
    c = _block_case(2, 0, mode, ard)
    r, xs = _dev(c["r"], "f64"), _dev(c["xs"], "f64")

    def run():
        blk = _make_block(ca, c, 0, mode, ard, linear=False)
        lml, dth, dz = blk.lml_grad(r)
        mean = torch.empty((NS, Q), dtype=torch.float64, device="cuda")
        var = torch.empty((NS,), dtype=torch.float64, device="cuda")
        blk.predict(xs, mean, var)
        return blk, lml, dth, dz, mean, var

    blk, lml, dth, dz, mean, var = run()
    lin_blk = _make_block(ca, c, 0, mode, ard)
    lin_blk.lml_grad(r)
    blk2, lml2, dth2, dz2, mean2, var2 = run()
    assert lml == lml2 and np.array_equal(dth, dth2) and dth.shape == (2 + np.size(c["ell"]),)
    assert torch.equal(_bits(dz), _bits(dz2)) and torch.equal(_bits(mean), _bits(mean2)) and torch.equal(_bits(var), _bits(var2))
    assert set(blk.grad_check) == {"closed", "pairwise"}
    assert abs(blk.grad_check["closed"] - blk.grad_check["pairwise"]) <= 1e-9 * abs(blk.grad_check["closed"])
    # the factor of K_uu by hand through the twin: the block's bits
    k = blk.kernel
    lu = dev.rbf_gram(blk._zs, k.l, k.sf, EPS * k.sf, lower_only=True, cov=k.cov)
    dev.potrf(lu, M)
    assert torch.equal(_bits(torch.tril(lu[:M, :M])), _bits(torch.tril(blk.lu[:M, :M])))
    # and the term is there: the linear block's factor differs
    assert not torch.equal(_bits(torch.tril(lin_blk.lu[:M, :M])), _bits(torch.tril(blk.lu[:M, :M])))


# ---- the plugin ------------------------------------------------------------------------------------------------------
def _plugin_data(d=2, n=1500, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d)) * np.array([1.0, 3.0, 0.5][:d]) + np.array([0.5, -1.0, 2.0][:d])
    y = np.stack([np.sin(2 * x[:, 0]) + 0.7 * x[:, -1], np.cos(x).prod(axis=1) - 0.3 * x[:, 0]], axis=1) + 0.1 * rng.normal(size=(n, 2))
    xs = rng.uniform(-2.2, 2.2, size=(NS, d)) * np.array([1.0, 3.0, 0.5][:d]) + np.array([0.5, -1.0, 2.0][:d])
    return x, y, xs


@pytest.mark.parametrize("approximation", ["vfe", "fitc"])
def test_plugin_predictions_against_the_oracle_through_the_z_scoring(ca, approximation):
    x, y, xs = _plugin_data()
    gp = ca.SparseGP_RBFLinear(num_inducing=150, lengthscale=[0.7, 1.3], variance=SF, linear_variance=[0.5, 0.2],
                               approximation=approximation)
    assert gp.fit([x, y]) is True
    assert np.array_equal(gp.linear_variances, [0.5, 0.2]) and np.array_equal(gp.lengthscales, [0.7, 1.3])
    mu, sd, ym, ys = x.mean(0), x.std(0), y.mean(0), y.std(0)
    xn, yn = (x - mu) / sd, (y - ym) / ys
    z = xn[gp.inducing_draw(x.shape[0])]
    noise = float(yn.var()) * 0.01
    mode = 1 if approximation == "vfe" else 0
    args = (xn, z, yn, 0, np.array([0.7, 1.3]), SF, noise, 1e-6, mode, np.array([0.5, 0.2]), (xs - mu) / sd)
    (wl, wm, wv), (dl, dm, dv) = sl.woodbury(*args), sl.dense(*args)
    mean, var = gp.predict_with_variance(xs)
    tol_m, tol_v = max(100 * _gap(wm, dm), 1e-9), max(100 * _gap(wv, dv), 1e-9)
    gm, gv = _gap(mean, wm * ys + ym), _gap(var, wv)
    print("plugin %s: mean %.2e (tol %.2e) var %.2e (%.2e)" % (approximation, gm, tol_m, gv, tol_v))
    assert gm <= tol_m and gv <= tol_v
    assert np.array_equal(gp.predict(xs), mean)
    _, var_n = gp.predict_with_variance(xs, include_noise=True)
    assert _gap(var_n, wv + noise) <= tol_v
    assert abs(gp.log_marginal_likelihood() - wl) <= max(100 * abs(wl - dl) / abs(dl), 1e-9) * abs(wl)
    for call in (lambda: gp.predictive_gradients(xs), lambda: gp.leave_one_out(), lambda: gp.loo_log_predictive_density(),
                 lambda: gp.predict_with_covariance(xs), lambda: gp.posterior_samples_f(xs)):
        with pytest.raises(TypeError, match="not yet supported"):
            call()


@pytest.mark.parametrize("ard", [True, False])
def test_plugin_gradient_against_central_differences_of_its_objective(ca, ard):
    x, y, _ = _plugin_data()
    gp = ca.SparseGP_RBFLinear(num_inducing=150, lengthscale=[0.7, 1.3] if ard else 0.9, variance=SF, linear_variance=[0.5, 0.2], ARD=ard)
    gp.fit([x, y])
    ell0 = gp.lengthscales if ard else np.array([gp.kernel.l])
    th0 = np.log(np.concatenate([[gp.kernel.sf], ell0, [gp.kernel.noise], gp.linear_variances]))
    lml, dth, dz = gp.log_marginal_likelihood_grad()
    assert lml == gp.log_marginal_likelihood() and dth.shape == th0.shape and dz.shape == (150, 2)

    def f(th):
        v = np.exp(th)
        ne = ell0.shape[0]
        return gp.log_marginal_likelihood(ell=v[1:1 + ne] if ard else float(v[1]), sf=v[0], noise=v[1 + ne], linear=v[2 + ne:])

    assert abs(f(th0) - lml) <= 1e-9 * abs(lml)
    step, cd = 1e-5, np.empty(th0.shape[0])
    for k in range(th0.shape[0]):
        hi, lo = th0.copy(), th0.copy()
        hi[k] += step
        lo[k] -= step
        cd[k] = (f(hi) - f(lo)) / (2 * step)
    gap = _gap(dth, cd)
    print("plugin gradient ard %d: gap to central differences %.2e (bound %.2e)" % (ard, gap, MARGIN * CENTRAL_LEVEL))
    assert gap <= MARGIN * CENTRAL_LEVEL
    # explicit arguments at the fitted values: the same call
    lml2, dth2, _ = gp.log_marginal_likelihood_grad(linear=gp.linear_variances, want_z=False)
    assert lml2 == lml and np.array_equal(dth2, dth)


@pytest.mark.parametrize("learn_z", [False, True])
def test_plugin_optimisers_do_not_lose_ground(ca, learn_z):
    x, y, _ = _plugin_data(n=800)
    start = ca.SparseGP_RBFLinear(num_inducing=60)
    start.fit([x, y])
    gp = ca.SparseGP_RBFLinear(num_inducing=60, optimize=True, jac="analytic", optimize_inducing=learn_z, max_iters=15)
    gp.fit([x, y])
    print("objective %.3f -> %.3f, linear variances %s" % (start.log_marginal_likelihood(), gp.log_marginal_likelihood(), gp.linear_variances))
    assert gp.log_marginal_likelihood() >= start.log_marginal_likelihood()
    v = gp.linear_variances
    assert v.shape == (2,) and np.isfinite(v).all() and (v > 0).all()
    assert gp.optimizer_result.x.shape[0] == 2 + 2 + 2 + (60 * 2 if learn_z else 0)
    assert not np.array_equal(v, start.linear_variances)


def test_plugin_extrapolates_a_trend_where_the_stationary_one_reverts(ca):
    """y = 1.5 x0 + sin(3 x0) + noise on [-1, 1]: at x0 = 2 the fitted RBF + Linear mean is closer to the noise-free target
    than SparseGP_RBF's on the same data and seed (the oracle pair differs by 1.5 there: tests/test_sparse_linear_host.py)."""
    x, y, target = sl.trend_problem(400, 0)
    with_term = ca.SparseGP_RBFLinear(num_inducing=60, seed=0)
    without = ca.SparseGP_RBF(num_inducing=60, seed=0, ARD=True)
    with_term.fit([x, y])
    without.fit([x, y])
    at = np.array([[2.0]])
    e_with = abs(float(with_term.predict(at)[0, 0]) - target(2.0))
    e_without = abs(float(without.predict(at)[0, 0]) - target(2.0))
    print("error at x0 = 2: with the term %.3f, without %.3f" % (e_with, e_without))
    assert e_with < e_without
