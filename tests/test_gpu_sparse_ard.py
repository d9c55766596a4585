"""GPU tests of the ARD length-scales of the sparse GP (include/cimrgp_sparse_ard.h; DESIGN.md, "ARD length-scales for the
sparse GP"): cimrgp_cov_pair_grad_ard against NumPy FP64 and against its twin, SparseBlock(lengthscales=).lml_grad against
the autograd oracle of tests/sparse_ard_numpy.py, the plugins' ARD keyword with fixed and learned parameters, and the
default path against the block driven by hand.

lml_grad is tested in FP64 only, as in tests/test_gpu_sparse_grad.py."""
import numpy as np
import pytest

import sparse_ard_numpy as sa
import sparse_grad_numpy as sg
import sparse_numpy as sn
from grad_numpy import kcov
from test_gpu_sparse import _plugin_inputs, _raw
from test_gpu_sparse_grad import ELL, PAIR_SHAPES, SF2, TDT, UNIT, _bits, _f32, _padded, sg_rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SF, NOISE, EPS = 1.3, 0.02, 1e-6
ELLS = (0.7, 1.3, 2.1)
NU = {0: None, 1: 0.5, 2: 1.5, 3: 2.5}


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


# ---- cimrgp_cov_pair_grad_ard ----------------------------------------------------------------------------------------
_PAIR = {}


def _pair_problem(na, nb, d, same, cov):
    """The inputs of tests/test_gpu_sparse_grad.py's pair test (FP32 holds them exactly; G of both signs over 1e-2 .. 1e2)
    with the ARD reference (NumPy, sparse_ard_numpy.pair_grad_ard)."""
    key = (na, nb, d, same, cov)
    if key not in _PAIR:
        rng = np.random.default_rng(na + 7 * nb + d)
        xa = _f32(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d))
        xb = xa if same else _f32(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d))
        g = _f32(rng.choice([-1.0, 1.0], size=(na, nb)) * 10.0 ** rng.uniform(-2, 2, size=(na, nb)))
        pre_s, pre_db = ((_f32(rng.normal(size=1 + d)), _f32(rng.normal(size=(nb, d)))) if same
                         else (np.zeros(1 + d), np.zeros((nb, d))))
        # the reference is evaluated in extended precision and rounded to FP64: at na = 1 the bound is 3 u, which the
        # roundings of a plain FP64 evaluation of the same formulae use up on their own
        ref, mag = sa.pair_grad_ard(xa, xb, g, cov, ELL, SF2, scale=-2.0 if same else 1.0, ft=np.longdouble)
        _PAIR[key] = (xa, xb, g, pre_s, pre_db, ref, mag, kcov(xa, xb, cov, ELL, SF2))
    return _PAIR[key]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("na,nb,d,same", PAIR_SHAPES)
def test_cov_pair_grad_ard_within_the_bound_and_against_its_twin(ca, dt, cov, na, nb, d, same):
    """The twin's bound per output, |err| <= ((na + 2) u + 4 kappa) sum |term| with kappa measured as there; and on the
    same inputs sums[0] and db are the twin's bits in FP64, the per-dimension sums add up to the twin's sums[1] within
    twice its bound (one bound for either side)."""
    dev, tdt = ca.device, TDT[dt]
    xa, xb, g, pre_s, pre_db, (s_ref, db_ref), (s_mag, db_mag), k_ref = _pair_problem(na, nb, d, same, cov)
    xad, xbd = torch.as_tensor(xa).to("cuda", tdt), torch.as_tensor(xb).to("cuda", tdt)
    kappa = float((np.abs(dev.rbf_cross(xad, xbd, ELL, SF2, cov=cov)[:na, :nb].double().cpu().numpy() - k_ref) / k_ref).max())
    gbuf = _padded(dev, g, tdt)
    scale = -2.0 if same else 1.0
    sums = torch.as_tensor(pre_s).to("cuda") if same else None
    db = torch.as_tensor(pre_db).to("cuda", tdt) if same else None
    sums, db = dev.cov_pair_grad_ard(xad, xbd, gbuf, ELL, SF2, scale=scale, accumulate=same, sums=sums, db=db, cov=cov)
    s, dbh = sums.cpu().numpy(), db.double().cpu().numpy()
    assert s.shape == (1 + d,) and dbh.shape == (nb, d)
    factor = (na + 2) * UNIT[dt] + 4 * kappa
    rs = np.abs(s - (s_ref + pre_s)) / (factor * (s_mag + np.abs(pre_s)) + 1e-300)
    rd = np.abs(dbh - (db_ref + pre_db)) / (factor * (db_mag + np.abs(pre_db)) + 1e-300)
    print("pair_grad_ard %s cov %d (%d, %d, %d)%s: kappa %.2e  err/bound sum k %.3e  sums l_e %.3e  db %.3e"
          % (dt, cov, na, nb, d, " same" if same else "", kappa, rs[0], rs[1:].max(), rd.max()))
    assert np.isfinite(s).all() and np.isfinite(dbh).all()
    assert rs.max() <= 1.0 and rd.max() <= 1.0
    # the twin on the same inputs (the preset of its sums[1]: the sum of the d presets)
    pre_t = np.array([pre_s[0], pre_s[1:].sum()])
    t_sums = torch.as_tensor(pre_t).to("cuda") if same else None
    t_db = torch.as_tensor(pre_db).to("cuda", tdt) if same else None
    t_sums, t_db = dev.cov_pair_grad(xad, xbd, gbuf, ELL, SF2, scale=scale, accumulate=same, sums=t_sums, db=t_db, cov=cov)
    ts = t_sums.cpu().numpy()
    bound_l = factor * (s_mag[1:].sum() + np.abs(pre_s[1:]).sum())
    print("    against the twin: sum k %s, db %s, sum_e against sums[1] %.3e of the bound"
          % (s[0] == ts[0], bool(torch.equal(_bits(t_db), _bits(db))), abs(s[1:].sum() - ts[1]) / (bound_l + 1e-300)))
    if dt == "f64":
        assert s[0] == ts[0] and torch.equal(_bits(t_sums[:1]), _bits(sums[:1])) and torch.equal(_bits(t_db), _bits(db))
    assert abs(s[1:].sum() - ts[1]) <= 2.0 * bound_l
    # either output alone gives the same bits
    if not same:
        s_only, none = dev.cov_pair_grad_ard(xad, xbd, gbuf, ELL, SF2, want_db=False, cov=cov)
        none2, db_only = dev.cov_pair_grad_ard(xad, xbd, gbuf, ELL, SF2, want_sums=False, cov=cov)
        assert none is None and none2 is None
        assert torch.equal(_bits(s_only), _bits(sums)) and torch.equal(_bits(db_only), _bits(db))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_cov_pair_grad_ard_is_bit_identical_run_to_run(ca, dt):
    dev, tdt = ca.device, TDT[dt]
    na, nb, d = 4097, 130, 3
    xa, xb, g = _pair_problem(na, nb, d, False, 2)[:3]
    xad, xbd = torch.as_tensor(xa).to("cuda", tdt), torch.as_tensor(xb).to("cuda", tdt)
    gbuf = _padded(dev, g, tdt)
    s1, d1 = dev.cov_pair_grad_ard(xad, xbd, gbuf, ELL, SF2, cov=2)
    s2, d2 = dev.cov_pair_grad_ard(xad, xbd, gbuf, ELL, SF2, cov=2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(d1), _bits(d2))


# ---- SparseBlock(lengthscales=).lml_grad -----------------------------------------------------------------------------
N, M, Q = 1500, 130, 2
_REF = {}


def _kernel(ca, cov, l=1.0):
    from cimrgp_amd.KernelClass import DenseMaternKernel, RBFKernel
    return RBFKernel(l=l, sf=SF, noise=NOISE) if cov == 0 else DenseMaternKernel(nu=NU[cov], l=l, sf=SF, noise=NOISE)


def _reference(d, cov, mode, ells):
    """(inputs, autograd oracle, gap of the two oracle forms (lml, theta, Z)) of sparse_grad_numpy.problem(1500, 130, d)."""
    key = (d, cov, mode, tuple(ells))
    if key not in _REF:
        x, z, r = sg.problem(N, M, d, seed=N + M + d + cov, q=Q)
        auto = sa.autograd(x, z, r, cov, ells, SF, NOISE, EPS, mode)
        lml, dth, dz = sa.chain(x, z, r, cov, ells, SF, NOISE, EPS, mode)
        gap = (abs(lml - auto[0]) / abs(auto[0]), sg_rel(dth, auto[1]), sg_rel(dz, auto[2]))
        _REF[key] = ((x, z, r), auto, gap)
    return _REF[key]


def _tol(gap):
    """The project's rule for lml_grad: 100 x the gap between the two oracle forms on the same inputs, floor 1e-9."""
    return tuple(max(1e-9, 100.0 * g) for g in gap)


def _block(ca, x, z, cov, mode, lengthscales=None, l=1.0):
    from cimrgp_amd.Sparse import SparseBlock
    to = lambda a: torch.as_tensor(a).to("cuda", torch.float64).contiguous()
    return SparseBlock(to(x), to(z), _kernel(ca, cov, l), 'fitc' if mode == 0 else 'vfe', EPS, lengthscales=lengthscales)


LML_GRAD_CASES = ([(d, cov, mode) for d in (2, 3) for cov in (0, 2) for mode in (0, 1)] + [(2, 1, 0), (2, 3, 0)])


@pytest.mark.parametrize("d,cov,mode", LML_GRAD_CASES)
def test_lml_grad_with_lengthscales_matches_the_autograd_oracle(ca, d, cov, mode):
    ells = ELLS[:d]
    (x, z, r), (l_ref, th_ref, z_ref), gap = _reference(d, cov, mode, ells)
    tol = _tol(gap)
    rd = torch.as_tensor(r).to("cuda")
    blk = _block(ca, x, z, cov, mode, ells)
    lml, dth, dz = blk.lml_grad(rd)
    assert dth.shape == (d + 2,) and tuple(dz.shape) == (M, d)
    err = (abs(lml - l_ref) / abs(l_ref), sg_rel(dth, th_ref), sg_rel(dz.cpu().numpy(), z_ref))
    check = blk.grad_check
    print("lml_grad ARD d %d cov %d mode %d: lml %.2e theta %.2e Z %.2e   tolerance %.2e %.2e %.2e   closed vs pairwise %.2e"
          % ((d, cov, mode) + err + tol + (abs(check["closed"] - check["pairwise"]) / abs(check["closed"]),)))
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]
    assert dth[0] == check["closed"] and abs(check["closed"] - check["pairwise"]) <= 2.0 ** -53 * M / EPS * abs(check["closed"])
    # the objective is fit()'s, bit for bit; theta alone: the same numbers, no dZ
    assert lml == _block(ca, x, z, cov, mode, ells).fit(rd).log_marginal_likelihood()
    lml_t, dth_t, none = _block(ca, x, z, cov, mode, ells).lml_grad(rd, want_z=False)
    assert none is None and lml_t == lml and np.array_equal(dth_t, dth)
    # x and z stay in the caller's units
    assert np.array_equal(blk.x.cpu().numpy(), x) and np.array_equal(blk.z.cpu().numpy(), z)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
def test_equal_lengthscales_against_the_isotropic_block(ca, cov, mode):
    """lengthscales = (0.5,) * d against l = 0.5.  RBF: the scaling by 2 is exact in every step, so the fit's LML and the
    predictive mean and variance are the isotropic block's bits.  Both covariances: everything within the 100 x gap rule,
    the d derivatives w.r.t. log l_e adding up to the isotropic one."""
    d = 3
    ells = (0.5,) * d
    (x, z, r), _, gap = _reference(d, cov, mode, ells)
    tol = _tol(gap)
    rd = torch.as_tensor(r).to("cuda")
    xs = torch.as_tensor(np.random.default_rng(3).uniform(-2.2, 2.2, size=(513, d))).to("cuda")
    out = []
    for kw in (dict(lengthscales=ells), dict(l=0.5)):
        blk = _block(ca, x, z, cov, mode, **kw).fit(rd)
        mean = torch.empty((513, Q), dtype=torch.float64, device="cuda")
        var = torch.empty(513, dtype=torch.float64, device="cuda")
        blk.predict(xs, mean, var, include_noise=True)
        lml_g, dth, dz = _block(ca, x, z, cov, mode, **kw).lml_grad(rd)
        out.append((blk.log_marginal_likelihood(), mean, var, lml_g, dth, dz.cpu().numpy()))
    (lml_a, mean_a, var_a, lg_a, th_a, dz_a), (lml_i, mean_i, var_i, lg_i, th_i, dz_i) = out
    folded = np.array([th_a[0], th_a[1:1 + d].sum(), th_a[-1]])
    err = (abs(lml_a - lml_i) / abs(lml_i), sg_rel(folded, th_i), sg_rel(dz_a, dz_i),
           float((mean_a - mean_i).abs().max()), float((var_a - var_i).abs().max()))
    print("equal length-scales cov %d mode %d: lml %.2e theta %.2e Z %.2e mean %.2e var %.2e   tolerance %.2e %.2e %.2e"
          % ((cov, mode) + err + tol))
    if cov == 0:
        assert lml_a == lml_i == lg_a == lg_i
        assert torch.equal(_bits(mean_a), _bits(mean_i)) and torch.equal(_bits(var_a), _bits(var_i))
    assert err[0] <= tol[0] and abs(lg_a - lg_i) <= tol[0] * abs(lg_i)
    assert err[1] <= tol[1] and err[2] <= tol[2]
    assert err[3] <= tol[0] * float(mean_i.abs().max()) and err[4] <= tol[0] * float(var_i.abs().max())


# ---- the plugins -----------------------------------------------------------------------------------------------------
def _cls(ca, mode):
    return ca.SGP_FITC if mode == 0 else ca.SparseGP_RBF


@pytest.mark.parametrize("mode", [0, 1])
def test_plugin_with_fixed_lengthscales_matches_the_numpy_woodbury_form(ca, mode):
    """Against sparse_numpy.woodbury on inputs divided by l, at 100 x its gap to sparse_numpy.dense on the same inputs,
    floor 1e-9."""
    n, m, d, ells = 1500, 130, 2, np.array([0.7, 1.3])
    x, y, xs = _raw(n, d, 5)
    g = _cls(ca, mode)(num_inducing=m, ARD=True, lengthscale=(0.7, 1.3), variance=SF)
    assert g.fit([x, y]) is True
    xz, z, yz, xsz, noise = _plugin_inputs(n, m, d, 5)
    assert abs(g.kernel.noise - noise) <= 1e-15 and g.kernel.l == 1.0 and np.array_equal(g.lengthscales, ells)
    assert g.block.lengthscales is not g.lengthscales and np.array_equal(g.block.lengthscales, ells)
    for include_noise in (False, True):
        lw, mw, vw = sn.woodbury(xz / ells, z / ells, yz, 0, 1.0, SF, noise, EPS, mode, xsz / ells, include_noise)
        ld, md, vd = sn.dense(xz / ells, z / ells, yz, 0, 1.0, SF, noise, EPS, mode, xsz / ells, include_noise)
        tol = tuple(max(1e-9, 100.0 * v) for v in (abs(lw - ld) / abs(ld), np.abs(mw - md).max(), np.abs(vw - vd).max()))
        mean, var = g.predict_with_variance(xs, include_noise=include_noise)
        mean_z = (mean - y.mean(axis=0)) / y.std(axis=0)
        gap = (abs(g.log_marginal_likelihood() - lw) / abs(lw), float(np.abs(mean_z - mw).max()), float(np.abs(var - vw).max()))
        print("ARD plugin mode %d noise %d: gap lml %.3e mean %.3e var %.3e   tolerance %.3e %.3e %.3e"
              % ((mode, include_noise) + gap + tol))
        assert gap[0] <= tol[0] and gap[1] <= tol[1] and gap[2] <= tol[2]
    assert np.array_equal(g.predict(xs), g.predict_with_variance(xs)[0])
    assert np.allclose(g.inducing_inputs, x[g.inducing_ids], rtol=0, atol=1e-12)
    # the gradient: (log sf, log l_1, log l_2, log noise); ell= takes a vector or a scalar
    lml, dth, dz = g.log_marginal_likelihood_grad()
    assert dth.shape == (4,) and dz.shape == (m, d) and lml == g.log_marginal_likelihood()
    assert g.log_marginal_likelihood(ell=(0.7, 1.3)) == lml
    l1, t1, _ = g.log_marginal_likelihood_grad(ell=0.9, want_z=False)
    l2, t2, _ = g.log_marginal_likelihood_grad(ell=(0.9, 0.9), want_z=False)
    assert l1 == l2 == g.log_marginal_likelihood(ell=0.9) and np.array_equal(t1, t2) and t1.shape == (4,)
    auto = sa.autograd(xz, z, yz, 0, ells, SF, noise, EPS, mode)
    chain = sa.chain(xz, z, yz, 0, ells, SF, noise, EPS, mode)
    gtol = _tol((0.0, sg_rel(chain[1], auto[1]), sg_rel(chain[2], auto[2])))
    print("ARD plugin mode %d gradient: theta %.2e Z %.2e   tolerance %.2e %.2e"
          % (mode, sg_rel(dth, auto[1]), sg_rel(dz, auto[2]), gtol[1], gtol[2]))
    assert sg_rel(dth, auto[1]) <= gtol[1] and sg_rel(dz, auto[2]) <= gtol[2]


def _learning_problem():
    """The ARD problem of tests/test_gpu_model.py, enlarged: the second input matters little, the third not at all."""
    rng = np.random.default_rng(31)
    n = 600
    x = rng.uniform(-2, 2, size=(n, 3))
    y = np.stack([np.sin(2.5 * x[:, 0]) + 0.2 * x[:, 1], np.cos(1.5 * x[:, 0]) * (1 + 0.1 * x[:, 1])], axis=1)
    y += 0.05 * rng.normal(size=y.shape)
    xt = rng.uniform(-1.8, 1.8, size=(50, 3))
    return x, y, xt


def _start_lml(g, y):
    yz = (y - y.mean(axis=0)) / y.std(axis=0)
    return g.log_marginal_likelihood(ell=1.0, sf=1.0, noise=float(yz.var()) * 0.01)


def test_plugin_learns_per_dimension_lengthscales(ca):
    x, y, xt = _learning_problem()
    g = ca.SGP_FITC(num_inducing=60, ARD=True, optimize=True, jac='analytic', max_iters=40)
    g.fit([x, y])
    start, end = _start_lml(g, y), g.log_marginal_likelihood()
    print("ARD learning: l = %s, LML %.2f -> %.2f in %d evaluations" % (g.lengthscales, start, end, g.optimizer_result.nfev))
    assert g.optimizer_result.x.shape == (5,) and g.lengthscales.shape == (3,) and g.kernel.l == 1.0
    assert np.array_equal(g.lengthscales, np.exp(g.optimizer_result.x[1:4]))
    assert end >= start
    assert g.lengthscales[2] > 5 * g.lengthscales[0]
    assert g.lengthscales[1] > g.lengthscales[0]
    assert np.isfinite(g.predict(xt)).all()


def test_plugin_two_point_optimiser_with_lengthscales(ca):
    x, y, xt = _learning_problem()
    g = ca.SGP_FITC(num_inducing=60, ARD=True, optimize=True, jac='2-point', max_iters=3)
    g.fit([x, y])
    mean, var = g.predict_with_variance(xt)
    assert g.optimizer_result.x.shape == (5,) and g.lengthscales.shape == (3,)
    assert np.isfinite(g.optimizer_result.x).all() and np.isfinite(g.log_marginal_likelihood())
    assert np.isfinite(mean).all() and np.isfinite(var).all() and (var >= 0).all()


def test_plugin_learns_inducing_inputs_with_lengthscales(ca):
    x, y, xt = _learning_problem()
    m = 60
    gz = ca.SGP_FITC(num_inducing=m, ARD=True, optimize=True, jac='analytic', optimize_inducing=True, max_iters=10)
    gz.fit([x, y])
    kz, ells = gz.kernel, gz.lengthscales
    zl = gz._z.cpu().numpy()
    xz, yz = (x - x.mean(axis=0)) / x.std(axis=0), (y - y.mean(axis=0)) / y.std(axis=0)
    z0 = xz[np.random.RandomState(0).permutation(600)[:m]]
    # the start: the objective at the constructor's values and the drawn Z (NumPy; the plugin now holds the learned Z)
    start = sn.woodbury(xz, z0, yz, 0, 1.0, 1.0, float(yz.var()) * 0.01, EPS, 0)[0]
    end = gz.log_marginal_likelihood()
    print("ARD learned Z: l = %s, LML %.2f -> %.2f, Z moved by %.3f" % (ells, start, end, np.abs(zl - z0).max()))
    assert gz.inducing_inputs.shape == (m, 3) and gz.optimizer_result.x.shape == (5 + m * 3,)
    assert np.array_equal(gz.optimizer_result.x[5:].reshape(m, 3), zl) and np.abs(zl - z0).max() > 0
    assert np.allclose(gz.inducing_inputs, zl * x.std(axis=0) + x.mean(axis=0), rtol=0, atol=1e-12)
    assert end >= start
    # the prediction uses the learned Z and l: a fixed-parameter plugin given both reproduces the mean (the noise of a plain
    # refit is the 1 % rule: the comparison goes through _block, as in tests/test_gpu_sparse_grad.py)
    back = ca.SGP_FITC(num_inducing=m, ARD=True, lengthscale=ells, variance=kz.sf, Z=gz.inducing_inputs)
    back.fit([x, y])
    assert back.optimize is False and np.array_equal(back.lengthscales, ells) and back.kernel.sf == kz.sf
    back.block = back._block(ells, kz.sf, kz.noise).fit(back._y)
    mean, mean_b = gz.predict(xt), back.predict(xt)
    xtz = (xt - x.mean(axis=0)) / x.std(axis=0)
    mw = sn.woodbury(xz / ells, zl / ells, yz, 0, 1.0, kz.sf, kz.noise, EPS, 0, xtz / ells)[1]
    md = sn.dense(xz / ells, zl / ells, yz, 0, 1.0, kz.sf, kz.noise, EPS, 0, xtz / ells)[1]
    tol = max(1e-9, 100.0 * float(np.abs(mw - md).max()))
    diff = float(np.abs((mean - mean_b) / y.std(axis=0)).max())
    print("ARD learned Z passed back: mean %.2e   tolerance %.2e" % (diff, tol))
    assert diff <= tol
    assert float(np.abs((mean - y.mean(axis=0)) / y.std(axis=0) - mw).max()) <= tol


# ---- the default -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_default_is_unchanged(ca, mode):
    """ARD not given, ARD=False given, and SparseBlock driven by hand: the same bits."""
    from cimrgp_amd.Sparse import SparseBlock
    n, m, d = 1500, 130, 2
    x, y, xs = _raw(n, d, 5)
    a = _cls(ca, mode)(num_inducing=m)
    b = _cls(ca, mode)(num_inducing=m, ARD=False)
    a.fit([x, y])
    b.fit([x, y])
    assert a.ARD is False and a.lengthscales is None and b.lengthscales is None and a.kernel.l == 1.0
    hand = SparseBlock(a._x, a._z, a._make_kernel(1.0, 1.0, a.kernel.noise), a.approximation, a.jitter).fit(a._y)
    assert a.log_marginal_likelihood() == b.log_marginal_likelihood() == hand.log_marginal_likelihood()
    (mean_a, var_a), (mean_b, var_b) = a.predict_with_variance(xs), b.predict_with_variance(xs)
    assert np.array_equal(mean_a, mean_b) and np.array_equal(var_a, var_b)
    xsd = torch.as_tensor((xs - x.mean(axis=0)) / x.std(axis=0)).to("cuda")
    mean_h = torch.empty((xs.shape[0], 2), dtype=torch.float64, device="cuda")
    var_h = torch.empty(xs.shape[0], dtype=torch.float64, device="cuda")
    hand.predict(xsd, mean_h, var_h)
    assert np.array_equal(mean_h.cpu().numpy() * y.std(axis=0) + y.mean(axis=0), mean_a)
    assert np.array_equal(var_h.cpu().numpy(), var_a)
    la, ta, za = a.log_marginal_likelihood_grad()
    lb, tb, zb = b.log_marginal_likelihood_grad()
    assert ta.shape == (3,) and la == lb and np.array_equal(ta, tb) and np.array_equal(za, zb)
