"""CPU tests of the gradients of the bound on uncertain inputs (include/cimrgp_psi_grad.h; DESIGN.md, "Gradients of the
bound on uncertain inputs"): the oracle of tests/psi_grad_numpy.py against central differences of tests/psi_numpy.py in
longdouble, the header's symbols, every refusal of the entry points that precedes a HIP call, the scratch sizes against
their Python restatement, and the argument checks of ``UncertainInputBlock`` and the ``BayesianGPLVM`` plugin."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import psi_grad_numpy as pg
import psi_numpy as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- the oracle against finite differences -----------------------------------------------------------------------------
#: The step and the allowance's floor, relative to the gradient's largest entry.  Measured here in longdouble: at h = 1e-4
#: every component of every case below passes with the floor at 0, the largest |analytic - D(h / 2)| being 6.3e-9 of the
#: largest entry -- the differences' own h^2 error, which ten times the step-halving estimate covers.  The floor guards a
#: component whose two differences agree by chance while the rounding of the longdouble bound (the two-sided solve by an
#: ill-conditioned K_uu) shows through the division by h: at h = 1e-5, where that noise dominates, it reaches 5.2e-9
#: (Z) and 1.0e-9 (s), so about 5e-10 at h = 1e-4; the floor is four times that.
FD_FLOOR = 2e-9
FD_STEP = 1e-4


def _problem(d):
    rng = np.random.RandomState(11 + d)
    mu, s, z = rng.randn(37, d), rng.uniform(0.01, 0.5, (37, d)), rng.randn(9, d)
    s[::5] = 0.0
    y = np.sin(mu @ rng.randn(d, 2)) + 0.1 * rng.randn(37, 2)
    return mu, s, z, y, np.array([0.8, 1.3][:d]), 1.4, 0.05


def _central(f, h):
    return (f(h) - f(-h)) / (2 * LD(h))


def _check(name, analytic, objective_at, scale):
    """``objective_at(step)``: the objective with the parameter moved by ``step``."""
    d1, d2 = _central(objective_at, FD_STEP), _central(objective_at, FD_STEP / 2)
    allow = 10 * abs(d1 - d2) + FD_FLOOR * scale
    err = abs(LD(analytic) - d2)
    print("%-14s analytic %+.12e  D(h/2) %+.12e  err %.2e  allowance %.2e  err/scale %.2e" % (
        name, float(analytic), float(d2), float(err), float(allow), float(err / scale)))
    assert err <= allow, name
    return float(err / scale)


def _entries(d):
    """(row, column) of the Z, mu and s entries that are moved: row 0 and row 5 have s = 0, row 3 and 36 have s > 0."""
    return [(0, 0), (4, d - 1), (8, 0)], [(0, 0), (3, d - 1), (36, 0)], [(0, 0), (5, d - 1), (3, 0), (36, d - 1)]


def _moved(a, idx, step):
    b = np.array(a, dtype=LD)
    b[idx] += LD(step)
    return b


def _cases(mu, s, z, ell, sf, grad, value):
    """(name, analytic, objective_at) over every parameter class of ``value(mu, s, z, ell, sf)``."""
    d = mu.shape[1]
    ze, me, se = _entries(d)
    up = lambda x, t: LD(x) * np.exp(LD(t))
    yield "log sf", grad['dsf'], lambda t: value(mu, s, z, ell, up(sf, t))
    for e in range(d):
        moved = lambda t, e=e: np.array([up(l, t) if i == e else LD(l) for i, l in enumerate(ell)], dtype=LD)
        yield "log l_%d" % e, grad['dl'][e], lambda t, moved=moved: value(mu, s, z, moved(t), sf)
    for idx in ze:
        yield "z%r" % (idx,), grad['dz'][idx], lambda t, idx=idx: value(mu, s, _moved(z, idx, t), ell, sf)
    for idx in me:
        yield "mu%r" % (idx,), grad['dmu'][idx], lambda t, idx=idx: value(_moved(mu, idx, t), s, z, ell, sf)
    for idx in se:
        yield "s%r (s = %g)" % (idx, s[idx]), grad['ds'][idx], lambda t, idx=idx: value(mu, _moved(s, idx, t), z, ell, sf)


@pytest.mark.parametrize("d", [1, 2])
def test_oracle_psi_contractions_equal_central_differences(d):
    mu, s, z, _, ell, sf, _ = _problem(d)
    assert s[0, 0] == 0.0 and s[5, d - 1] == 0.0 and s[3, 0] > 0
    rng = np.random.RandomState(5)
    g1 = rng.randn(37, 9)
    g2 = rng.randn(9, 9)
    g2 = g2 + g2.T
    worst = 0.0
    for which, g, psi, psi_grad in (("psi1", g1, po.psi1, pg.psi1_grad), ("psi2", g2, po.psi2, pg.psi2_grad)):
        a = psi_grad(mu, s, z, ell, sf, g, LD)
        grad = dict(dsf=a['sums'][0], dl=a['sums'][1:], dz=a['dz'], dmu=a['dmu'], ds=a['ds'])
        scale = max(float(np.abs(v).max()) for v in grad.values())
        value = lambda mu_, s_, z_, ell_, sf_: (np.asarray(g, dtype=LD) * psi(mu_, s_, z_, ell_, sf_, LD)).sum()
        for name, analytic, at in _cases(mu, s, z, ell, sf, grad, value):
            worst = max(worst, _check(which + " " + name, analytic, at, scale))
    print("d = %d: largest error relative to the largest entry %.2e" % (d, worst))


@pytest.mark.parametrize("d", [1, 2])
def test_oracle_bound_gradient_equals_central_differences(d):
    mu, s, z, y, ell, sf, noise = _problem(d)
    f, grad = pg.bound_grad(mu, s, z, y, ell, sf, noise, ft=LD)
    assert f == po.Model(mu, s, z, y, ell, sf, noise, ft=LD).bound
    scale = max(float(np.abs(np.asarray(v)).max()) for v in grad.values())
    value = lambda mu_, s_, z_, ell_, sf_, noise_=noise: po.Model(mu_, s_, z_, y, ell_, sf_, noise_, ft=LD).bound
    worst = 0.0
    for name, analytic, at in _cases(mu, s, z, ell, sf, grad, value):
        worst = max(worst, _check(name, analytic, at, scale))
    worst = max(worst, _check("log noise", grad['dnoise'], lambda t: value(mu, s, z, ell, sf, LD(noise) * np.exp(LD(t))), scale))
    print("d = %d: largest error relative to the largest entry %.2e" % (d, worst))


def test_oracle_kl_gradient_and_elbo():
    mu, s, z, y, ell, sf, noise = _problem(2)
    pm, pv = mu + 0.1, np.full(mu.shape, 0.3)
    for prior in ((None, None), (pm, pv)):
        kl, kmu, ks = pg.kl_parts(mu, s, *prior, ft=LD)
        assert (kmu[s == 0] == 0).all() and (ks[s == 0] == 0).all()
        scale = max(float(np.abs(kmu).max()), float(np.abs(ks).max()))
        for idx in ((3, 0), (36, 1)):
            _check("kl mu%r" % (idx,), kmu[idx], lambda t, idx=idx: pg.kl_parts(_moved(mu, idx, t), s, *prior, ft=LD)[0], scale)
            _check("kl s%r" % (idx,), ks[idx], lambda t, idx=idx: pg.kl_parts(mu, _moved(s, idx, t), *prior, ft=LD)[0], scale)
    # the default prior is psi_numpy's KL; the prior N(mu, s) itself gives 0
    assert abs(pg.kl_parts(mu, s, ft=LD)[0] - po.Model(mu, s, z, y, ell, sf, noise, ft=LD).kl) <= 1e-15
    assert pg.kl_parts(mu, s, mu, np.where(s > 0, s, 1.0), ft=LD)[0] == 0
    f, g = pg.elbo_grad(mu, s, z, y, ell, sf, noise, prior_mean=pm, prior_var=pv)
    f0, g0 = pg.bound_grad(mu, s, z, y, ell, sf, noise)
    kl, kmu, ks = pg.kl_parts(mu, s, pm, pv)
    assert f == f0 - kl and (g['dmu'] == g0['dmu'] - kmu).all() and (g['ds'] == g0['ds'] - ks).all() and (g['dz'] == g0['dz']).all()


def test_the_rounding_bounds_are_finite_and_cover_the_stored_value():
    mu, s, z, _ = po.problem(41, 11, 3, 5)
    ell, sf = [0.8, 1.3, 1.0], 1.4
    rng = np.random.RandomState(2)
    g1, g2 = rng.randn(41, 11), rng.randn(11, 11)
    g2 = g2 + g2.T
    for grad, g in ((pg.psi1_grad, g1), (pg.psi2_grad, g2)):
        val, wts = grad(mu, s, z, ell, sf, g, LD), grad(mu, s, z, ell, sf, g, LD, bound=True)
        for key in ("dmu", "ds", "dz", "sums"):
            for u in (2.0 ** -53, 2.0 ** -24):
                b = pg.grad_bound(val[key], wts[key], u)
                assert b.shape == np.shape(val[key]) and np.isfinite(b).all(), key
                assert (b >= u * np.abs(np.asarray(val[key], dtype=np.float64))).all() and (b > 0).all(), key


# ---- the header -------------------------------------------------------------------------------------------------------
P1G, P2G = 'cimrgp_psi1_grad', 'cimrgp_psi2_grad'


def test_psi_grad_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_psi_grad.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == [P1G, P1G + "_scratch_bytes", P2G, P2G + "_scratch_bytes"]
    assert sorted(_lib.PSI_GRAD_SIGNATURES) == names
    for name in names:
        assert getattr(lib, name).argtypes == _lib.PSI_GRAD_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.PSI_GRAD_SIGNATURES[name][0], name
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert main.index('#include "cimrgp_psi.h"') < main.index('#include "cimrgp_psi_grad.h"')
    order = list(_lib.HEADERS)
    assert order.index("cimrgp_psi_grad.h") == order.index("cimrgp_psi.h") + 1
    assert " psi_grad " in open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    assert int(re.search(r"#define CIMRGP_PSI_GRAD_ROW_WGS (\d+)", text).group(1)) == _lib.PSI_GRAD_ROW_WGS
    # the helpers the three sources need live in one header, and none of the sources keeps a copy of its own
    csrc = os.path.join(ROOT, "cimrgp_amd", "csrc")
    common = open(os.path.join(csrc, "psi_common.hpp")).read()
    sources = {name: open(os.path.join(csrc, name)).read() for name in ("psi.hip", "psi_grad.hip", "psi_rows.hip")}
    for helper in ("with_dim_exact(int d", "psi_slice_len(int64_t n", "void psi2_tile_of(int tile", "t_exp(double x)",
                   "void k_psi2_rows(const T* __restrict__ mu", "psi2_rows_bytes(int dtype", "T psi_ordered_sum(const T* __restrict__ part",
                   "void psi2_count_bad(const double* __restrict__ badpart", "T psi1_row_consts(const T* __restrict__ mu",
                   "T psi1_exponent(T c0, const T* mv, const T* z, const T* hr, T* df)", "T psi2_exponent(T c0",
                   "T psi2_own_row(const T* __restrict__ rc", "void psi2_stage_points(const T* __restrict__ z",
                   "void psi2_stage_chunk(T* lds", "void psi2_pair_points(const T* __restrict__ z"):
        assert common.count(helper) == 1, helper
        for name, text in sources.items():
            assert helper not in text, (name, helper)
    for name, text in sources.items():
        # one pass over the rows for every Psi2 call; the bad-row count and the chunk staging are written in the header only
        assert "k_psi2g_rows" not in text and "psirq_rc_bytes" not in text, name
        assert "b += badpart[i]" not in text and "rc[(int64_t)kb * RS + idx]" not in text, name
        assert "log1p(" not in text and "dl * dl" not in text and "(T)0.5 * z[" not in text, name
        assert "rc[(int64_t)i * RS + D + e]" not in text, name
        assert '#include "psi_common.hpp"' in text, name
    assert common.count("b += badpart[i]") == 1 and "lds_settle(lds + idx)" in common


# ---- refusals --------------------------------------------------------------------------------------------------------
_HEAD = [('dtype', 1), ('mu', 'P'), ('s', 'P'), ('z', 'P'), ('n', 600), ('m', 100), ('d', 2), ('ell', 'P'), ('sf2', 1.3), ('g', 'P'),
         ('ldg', 112), ('dmu', 'P'), ('ds', 'P'), ('dz', 'P'), ('sums', 'P'), ('scratch', 'P')]
BASE = {
    P1G: _HEAD + [('scratch_bytes', 1 << 40), ('stream', None)],
    P2G: _HEAD + [('scratch_bytes', 1 << 40), ('bad', 'P'), ('stream', None)],
}


def _rows(fn, pointers, short):
    rows = [(fn, {'dtype': 7}, -1, 'unknown dtype')]
    rows += [(fn, {p: None}, -1, 'null pointer') for p in pointers]
    rows += [(fn, {'n': 0}, -1, 'n must be in [1, 16777216]'), (fn, {'n': (1 << 24) + 1}, -1, 'n must be in [1, 16777216]'),
             (fn, {'m': 0}, -1, 'm must be in [1, 16384]'), (fn, {'m': 16385, 'ldg': 16400}, -1, 'm must be in [1, 16384]'),
             (fn, {'d': 0}, -1, 'input dimension must be in [1, 8]'), (fn, {'d': 9}, -1, 'input dimension must be in [1, 8]'),
             (fn, {'sf2': 0.0}, -1, 'sf2 must be positive'), (fn, {'sf2': float('nan')}, -1, 'sf2 must be positive'),
             (fn, {'ldg': 99}, -1, 'leading dimension too small'),
             (fn, {'scratch': 'P+8'}, -1, 'scratch must be 16-byte aligned'),
             (fn, {'scratch_bytes': short}, -1, 'scratch too small'), (fn, {'scratch_bytes': 0}, -1, 'scratch too small'),
             (fn, {'dtype': 7, 'mu': None, 'n': 0, 'd': 0}, -1, 'unknown dtype')]
    return [(name, broken, status, '%s: %s' % (name, text)) for name, broken, status, text in rows]


_POINTERS = ['mu', 's', 'z', 'ell', 'g', 'dmu', 'ds', 'dz', 'sums', 'scratch']
ROWS = _rows(P1G, _POINTERS, 'one short 1') + _rows(P2G, _POINTERS + ['bad'], 'one short 2')


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+8": p + 8, "one short 1": lib.cimrgp_psi1_grad_scratch_bytes(1, 600, 100, 2) - 1,
                 "one short 2": lib.cimrgp_psi2_grad_scratch_bytes(1, 600, 100, 2) - 1}


def test_psi_grad_refusals_status_and_text():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    assert stand_in["one short 1"] > 0 and stand_in["one short 2"] > 0
    for name in BASE:
        assert len(BASE[name]) == len(_lib.PSI_GRAD_SIGNATURES[name][1]), name
    for name, broken, status, text in ROWS:
        assert broken and set(broken) <= {k for k, _ in BASE[name]}, broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_every_check_of_the_grad_entry_points_has_a_row():
    """Each CIMRGP_REQUIRE text of psi_grad.hip's entry points occurs in the table under its function's name."""
    src = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "psi_grad.hip")).read()
    ext = src[src.index('extern "C" {'):]
    seen = {(name, text.split(': ', 1)[1]) for name, _, _, text in ROWS}
    for name in BASE:
        body = ext[ext.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        checks = re.findall(r'CIMRGP_REQUIRE\(.*?, fn,\s*"([^"]+)"\);', body, re.S)
        assert len(checks) == 9, name
        for what in checks:
            assert (name, what) in seen, (name, what)
        # every check stands before the first launch
        assert body.rindex("CIMRGP_REQUIRE") < body.index("with_dtype(")


def test_scratch_bytes_are_the_python_restatement():
    lib = _lib.load()
    for n, m in ((1, 1), (63, 64), (64, 65), (150, 40), (255, 63), (300, 65), (257, 130), (4097, 100), (65536, 100), (65536, 1000),
                 (1 << 24, 16384), (1 << 24, 1)):
        for dtype, esz in ((0, 4), (1, 8)):
            for d in (1, 2, 3, 8):
                got1, got2 = lib.cimrgp_psi1_grad_scratch_bytes(dtype, n, m, d), lib.cimrgp_psi2_grad_scratch_bytes(dtype, n, m, d)
                assert got1 == pg.psi1_grad_scratch_bytes(esz, n, m, d) and got1 % 16 == 0, (n, m, d, dtype)
                assert got2 == pg.psi2_grad_scratch_bytes(esz, n, m, d) and got2 % 16 == 0, (n, m, d, dtype)
    # the one-pass design's n x tiles x 2 d partial sums are not there: well under 100 MB at the flagship size, d = 8
    assert lib.cimrgp_psi2_grad_scratch_bytes(1, 65536, 1000, 8) < 100e6
    for fn in (lib.cimrgp_psi1_grad_scratch_bytes, lib.cimrgp_psi2_grad_scratch_bytes):
        for bad in ((7, 10, 10, 2), (1, 0, 10, 2), (1, 10, 0, 2), (1, 10, 10, 0), (1, 10, 10, 9), (1, (1 << 24) + 1, 10, 2), (1, 10, 16385, 2)):
            assert fn(*bad) == 0, bad


# ---- the block and the plugin ------------------------------------------------------------------------------------------
def test_block_prior_arguments_and_refusals_before_a_fit():
    torch = pytest.importorskip("torch")
    from cimrgp_amd import UncertainInputBlock
    from cimrgp_amd.KernelClass import RBFKernel
    f64 = torch.float64
    mu = torch.arange(30, dtype=f64).reshape(10, 3) / 10
    z = torch.zeros((4, 3), dtype=f64)
    k = RBFKernel(l=0.7, sf=1.3, noise=0.5)
    s = torch.full((10, 3), 0.5, dtype=f64)
    s[::2] = 0.0
    pm, pv = mu.numpy() + 0.1, np.full((10, 3), 0.3)
    for kw in (dict(prior_mean=torch.zeros((9, 3), dtype=f64)), dict(prior_var=torch.zeros((10, 3), dtype=f64)),
               dict(prior_var=torch.full((10, 3), -1.0, dtype=f64)), dict(prior_mean=torch.full((10, 3), float('nan'), dtype=f64))):
        with pytest.raises(ValueError, match="prior"):
            UncertainInputBlock(mu, s, z, k, **kw)
    blk = UncertainInputBlock(mu, s, z, k, prior_mean=torch.as_tensor(pm), prior_var=torch.as_tensor(pv))
    want = float(pg.kl_parts(mu.numpy(), s.numpy(), pm, pv)[0])
    assert abs(blk.kl() - want) <= 1e-13 * abs(want)
    # a shared variance under a given prior
    shared = UncertainInputBlock(mu, [0.5, 0.0, 2.0], z, k, prior_mean=torch.as_tensor(pm), prior_var=torch.as_tensor(pv))
    want = float(pg.kl_parts(mu.numpy(), np.broadcast_to([0.5, 0.0, 2.0], (10, 3)), pm, pv)[0])
    assert abs(shared.kl() - want) <= 1e-13 * abs(want)
    # the default is today's KL
    assert UncertainInputBlock(mu, s, z, k).kl() == UncertainInputBlock(mu, s, z, k, prior_mean=None, prior_var=None).kl()
    for call in (lambda b: b.bound_grad(), lambda b: b.elbo_grad()):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
            call(blk)
    with pytest.raises(TypeError, match="not yet supported"):
        blk.lml_grad(torch.zeros((10, 2), dtype=f64))


def test_gplvm_plugin_argument_checks_and_export():
    import inspect
    import cimrgp_amd
    from cimrgp_amd import BGPLVM
    from cimrgp_amd.GPLVM import BayesianGPLVM
    assert 'BayesianGPLVM' not in cimrgp_amd.__all__ and issubclass(BayesianGPLVM, BGPLVM) and BayesianGPLVM.name == 'BayesianGPLVM'
    sig = inspect.signature(BayesianGPLVM.__init__).parameters
    parent = inspect.signature(BGPLVM.__init__).parameters
    assert list(sig) == list(parent) + ['jac', 'optimize_inducing', 'optimize_inputs', 'input_prior']
    assert [sig[k].default for k in list(sig)[1:]] == [parent[k].default for k in list(parent)[1:]] + ['analytic', False, False, 'observed']
    for kw in (dict(jac='3-point'), dict(input_prior='flat'), dict(optimize_inducing=True), dict(optimize_inputs=True),
               dict(optimize=True, jac='2-point', optimize_inducing=True), dict(optimize=True, jac='2-point', optimize_inputs=True),
               dict(num_inducing=0), dict(noise=0.0), dict(X_var=-0.1)):
        with pytest.raises(ValueError):
            BayesianGPLVM(**kw)
    g = BayesianGPLVM(optimize=True, optimize_inducing=True, optimize_inputs=True)
    assert g.input_means is None and g.input_variances is None
    xs = np.zeros((3, 2))
    for name, args in (("predict", (xs,)), ("elbo", ()), ("elbo_grad", ()), ("kl_divergence", ())):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
            getattr(g, name)(*args)
    with pytest.raises(TypeError, match="not yet supported"):
        g.predict_with_variance(xs, test_var=0.1)
    for name, args in (("predictive_gradients", (xs,)), ("leave_one_out", ()), ("predict_with_covariance", (xs,))):
        with pytest.raises(TypeError, match="not yet supported"):
            getattr(g, name)(*args)
