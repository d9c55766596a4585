"""CPU tests of the sparse GP on uncertain inputs (include/cimrgp_psi.h; DESIGN.md, "Sparse GP regression on uncertain
inputs"): the header's symbols, every refusal of the entry points that precedes a HIP call, the header's slice rule and
scratch size, the argument checks of ``UncertainInputBlock`` and the ``BGPLVM`` plugin, and the oracle of
tests/psi_numpy.py: its closed forms against a Gauss-Hermite evaluation of E[k] and E[k^T k], the limits at s = 0, the
shared-variance factorisation, and the bound at s = 0 against the VFE bound of tests/sparse_numpy.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import psi_numpy as po
import sparse_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psi_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_psi.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_psi1", "cimrgp_psi2", "cimrgp_psi2_scratch_bytes", "cimrgp_psi2_slices"]
    assert sorted(_lib.PSI_SIGNATURES) == names
    for name in names:
        assert getattr(lib, name).argtypes == _lib.PSI_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.PSI_SIGNATURES[name][0], name
    assert '#include "cimrgp_psi.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert " psi " in open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    # the header's constants are the table's
    for macro, value in (("TILE", _lib.PSI2_TILE), ("TARGET_WGS", _lib.PSI2_TARGET_WGS), ("MIN_SLICE", _lib.PSI2_MIN_SLICE),
                         ("SLICE_ALIGN", _lib.PSI2_SLICE_ALIGN)):
        assert int(re.search(r"#define CIMRGP_PSI2_%s (\d+)" % macro, text).group(1)) == value


# ---- refusals --------------------------------------------------------------------------------------------------------
P1, P2 = 'cimrgp_psi1', 'cimrgp_psi2'
BASE = {
    P1: [('dtype', 1), ('mu', 'P'), ('s', 'P'), ('z', 'P'), ('n', 600), ('m', 100), ('d', 2), ('ell', 'P'), ('sf2', 1.3),
         ('out', 'P'), ('ldo', 112), ('stream', None)],
    P2: [('dtype', 1), ('mu', 'P'), ('s', 'P'), ('z', 'P'), ('n', 600), ('m', 100), ('d', 2), ('ell', 'P'), ('sf2', 1.3),
         ('c', 'P'), ('ldc', 112), ('scratch', 'P'), ('scratch_bytes', 1 << 40), ('bad', 'P'), ('stream', None)],
}
ROWS = [
    (P1, {'dtype': 7}, -1, 'cimrgp_psi1: unknown dtype'),
    (P1, {'mu': None}, -1, 'cimrgp_psi1: null pointer'),
    (P1, {'s': None}, -1, 'cimrgp_psi1: null pointer'),
    (P1, {'z': None}, -1, 'cimrgp_psi1: null pointer'),
    (P1, {'ell': None}, -1, 'cimrgp_psi1: null pointer'),
    (P1, {'out': None}, -1, 'cimrgp_psi1: null pointer'),
    (P1, {'n': -1}, -1, 'cimrgp_psi1: n must be in [0, 2^31)'),
    (P1, {'n': 1 << 31}, -1, 'cimrgp_psi1: n must be in [0, 2^31)'),
    (P1, {'m': 0}, -1, 'cimrgp_psi1: m must be in [1, 2^31)'),
    (P1, {'m': 1 << 31, 'ldo': 1 << 31}, -1, 'cimrgp_psi1: m must be in [1, 2^31)'),
    (P1, {'d': 0}, -1, 'cimrgp_psi1: input dimension must be in [1, 8]'),
    (P1, {'d': 9}, -1, 'cimrgp_psi1: input dimension must be in [1, 8]'),
    (P1, {'sf2': 0.0}, -1, 'cimrgp_psi1: sf2 must be positive'),
    (P1, {'sf2': float('nan')}, -1, 'cimrgp_psi1: sf2 must be positive'),
    (P1, {'ldo': 99}, -1, 'cimrgp_psi1: leading dimension too small'),
    (P1, {'dtype': 7, 'mu': None, 'n': -1, 'd': 0}, -1, 'cimrgp_psi1: unknown dtype'),
    (P2, {'dtype': 7}, -1, 'cimrgp_psi2: unknown dtype'),
    (P2, {'mu': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'s': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'z': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'ell': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'c': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'scratch': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'bad': None}, -1, 'cimrgp_psi2: null pointer'),
    (P2, {'n': 0}, -1, 'cimrgp_psi2: n must be in [1, 16777216]'),
    (P2, {'n': (1 << 24) + 1}, -1, 'cimrgp_psi2: n must be in [1, 16777216]'),
    (P2, {'m': 0}, -1, 'cimrgp_psi2: m must be in [1, 16384]'),
    (P2, {'m': 16385, 'ldc': 16400}, -1, 'cimrgp_psi2: m must be in [1, 16384]'),
    (P2, {'d': 0}, -1, 'cimrgp_psi2: input dimension must be in [1, 8]'),
    (P2, {'d': 9}, -1, 'cimrgp_psi2: input dimension must be in [1, 8]'),
    (P2, {'sf2': 0.0}, -1, 'cimrgp_psi2: sf2 must be positive'),
    (P2, {'ldc': 99}, -1, 'cimrgp_psi2: leading dimension too small'),
    (P2, {'scratch': 'P+8'}, -1, 'cimrgp_psi2: scratch must be 16-byte aligned'),
    (P2, {'scratch_bytes': 'one short'}, -1, 'cimrgp_psi2: scratch too small'),
    (P2, {'scratch_bytes': 0}, -1, 'cimrgp_psi2: scratch too small'),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+8": p + 8, "one short": _lib.load().cimrgp_psi2_scratch_bytes(1, 600, 100, 2) - 1}


def test_psi_refusals_status_and_text():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name in BASE:
        assert len(BASE[name]) == len(_lib.PSI_SIGNATURES[name][1]), name
    for name, broken, status, text in ROWS:
        assert broken and set(broken) <= {k for k, _ in BASE[name]}, broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)
    # nothing to do: status 0 without a launch
    assert lib.cimrgp_psi1(*_args(P1, {'n': 0}, stand_in)) == 0, _lib.last_error()


def test_every_check_of_the_entry_points_has_a_row():
    """Each CIMRGP_REQUIRE text of psi.hip's entry points occurs in the table under its function's name."""
    src = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "psi.hip")).read()
    ext = src[src.index('extern "C" {'):]
    seen = {(name, text.split(': ', 1)[1]) for name, _, _, text in ROWS}
    for name in BASE:
        body = ext[ext.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        checks = re.findall(r'CIMRGP_REQUIRE\(.*?, fn,\s*"([^"]+)"\);', body, re.S)
        assert len(checks) >= 7, name
        for what in checks:
            assert (name, what) in seen, (name, what)


def test_slice_rule_and_scratch_bytes_are_the_headers():
    lib = _lib.load()
    for n, m in ((1, 1), (63, 64), (64, 65), (150, 40), (255, 63), (300, 65), (257, 130), (4097, 100), (65536, 100), (65536, 1000),
                 (1 << 24, 16384), (1 << 24, 1)):
        s, length = po.slices(n, m)
        assert lib.cimrgp_psi2_slices(n, m) == s, (n, m)
        assert (s - 1) * length < n <= s * length and length % _lib.PSI2_SLICE_ALIGN == 0
        for dtype, esz in ((0, 4), (1, 8)):
            for d in (1, 3, 8):
                assert lib.cimrgp_psi2_scratch_bytes(dtype, n, m, d) == po.scratch_bytes(esz, n, m, d), (n, m, d, dtype)
    # n = 150 cuts into three slices of 64 rows, the last one ragged (22 rows)
    assert po.slices(150, 40) == (3, 64)
    # outside the limits, or an unknown dtype: 0
    assert lib.cimrgp_psi2_slices(0, 10) == 0 and lib.cimrgp_psi2_slices(10, 16385) == 0 and lib.cimrgp_psi2_slices((1 << 24) + 1, 1) == 0
    for bad in ((7, 10, 10, 2), (1, 0, 10, 2), (1, 10, 0, 2), (1, 10, 10, 0), (1, 10, 10, 9)):
        assert lib.cimrgp_psi2_scratch_bytes(*bad) == 0, bad


# ---- the block and the plugin ------------------------------------------------------------------------------------------
def test_block_argument_checks():
    torch = pytest.importorskip("torch")
    from cimrgp_amd import UncertainInputBlock
    from cimrgp_amd.KernelClass import DenseMaternKernel, RBFKernel
    f64 = torch.float64
    x, z = torch.zeros((10, 3), dtype=f64), torch.zeros((4, 3), dtype=f64)
    k = RBFKernel(l=0.7, sf=1.3, noise=0.5)
    with pytest.raises(TypeError, match="not yet supported"):
        UncertainInputBlock(x, 0.1, z, DenseMaternKernel(nu=1.5, l=0.7, sf=1.3, noise=0.5))
    with pytest.raises(TypeError, match="not yet supported"):
        UncertainInputBlock(x.float(), 0.1, z.float(), k)
    with pytest.raises(ValueError, match="positive noise"):
        UncertainInputBlock(x, 0.1, z, RBFKernel(l=0.7, sf=1.3))
    for bad in (-0.1, float('nan'), [0.1, 0.2], [0.1, 0.2, float('inf')], torch.zeros((9, 3), dtype=f64), torch.zeros((10, 3))):
        with pytest.raises(ValueError, match="x_var"):
            UncertainInputBlock(x, bad, z, k)
    with pytest.raises(ValueError, match="lengthscales"):
        UncertainInputBlock(x, 0.1, z, RBFKernel(l=1.0, sf=1.3, noise=0.5), lengthscales=[1.0, 2.0])
    blk = UncertainInputBlock(x, [0.1, 0.0, 0.2], z, RBFKernel(l=1.0, sf=1.3, noise=0.5), lengthscales=[1.0, 2.0, 3.0])
    assert blk.approximation == 'vfe' and blk.x_var.shape == (3,) and list(blk.ell) == [1.0, 2.0, 3.0]
    assert isinstance(UncertainInputBlock(x, torch.zeros((10, 3), dtype=f64), z, k).x_var, torch.Tensor)
    xs, r = torch.zeros((5, 3), dtype=f64), torch.zeros((10, 2), dtype=f64)
    for call in (lambda b: b.bound(), lambda b: b.elbo(), lambda b: b.predict(xs, None, None), lambda b: b.predict(xs, r[:5], None, xs_var=0.1)):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
            call(blk)
    for call in (lambda b: b.predict(xs, None, xs[:, 0], xs_var=0.1), lambda b: b.predict_grad(xs, None, None), lambda b: b.loo(r, None, None),
                 lambda b: b.joint(xs), lambda b: b.lml_grad(r), lambda b: b.fit_layer(r, r, r), lambda b: b.predict_layer(xs, r)):
        with pytest.raises(TypeError, match="not yet supported"):
            call(blk)
    # the KL term needs no device: the entries with s = 0 are observed inputs and add nothing
    mu = torch.arange(30, dtype=f64).reshape(10, 3) / 10
    s = torch.full((10, 3), 0.5, dtype=f64)
    s[::2] = 0.0
    want = po.Model(mu.numpy(), s.numpy(), z.numpy() + np.arange(4)[:, None], np.zeros((10, 1)), 0.7, 1.3, 0.5).kl
    assert abs(UncertainInputBlock(mu, s, z, k).kl() - float(want)) <= 1e-13 * abs(float(want))
    shared = UncertainInputBlock(mu, [0.5, 0.0, 2.0], z, k).kl()
    want = po.Model(mu.numpy(), np.array([0.5, 0.0, 2.0]), z.numpy() + np.arange(4)[:, None], np.zeros((10, 1)), 0.7, 1.3, 0.5).kl
    assert abs(shared - float(want)) <= 1e-13 * abs(float(want))
    assert UncertainInputBlock(mu, 0.0, z, k).kl() == 0.0


def test_plugin_argument_checks_and_export():
    import inspect
    import cimrgp_amd
    from cimrgp_amd import BGPLVM, RegressionMethod
    assert 'BGPLVM' in cimrgp_amd.__all__ and 'UncertainInputBlock' in cimrgp_amd.__all__
    assert BGPLVM.name == 'BGPLVM' and issubclass(BGPLVM, RegressionMethod)
    sig = inspect.signature(BGPLVM.__init__).parameters
    assert list(sig) == ['self', 'num_inducing', 'X_var', 'noise', 'lengthscale', 'variance', 'ARD', 'Z', 'seed', 'jitter', 'device',
                         'optimize', 'max_iters']
    # the reference's defaults
    assert [sig[k].default for k in list(sig)[1:]] == [100, None, 1.0, 1., 1., True, None, 0, 1e-6, None, False, 200]
    assert list(inspect.signature(BGPLVM.predict_with_variance).parameters)[:4] == ['self', 'test_data', 'include_noise', 'test_var']
    for kw in (dict(num_inducing=0), dict(noise=0.0), dict(noise=[1.0]), dict(variance=-1.0), dict(lengthscale=0.0),
               dict(lengthscale=[1.0, -1.0]), dict(lengthscale=[1.0, 2.0], ARD=False), dict(lengthscale=[[1.0]]), dict(jitter=-1.0),
               dict(X_var=-0.1), dict(X_var=[0.1, float('nan')]), dict(X_var=np.zeros((2, 2, 2)))):
        with pytest.raises(ValueError):
            BGPLVM(**kw)
    g = BGPLVM()
    xs = np.zeros((3, 2))
    for name, args in (("predict", (xs,)), ("predict_with_variance", (xs,)), ("elbo", ()), ("kl_divergence", ())):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
            getattr(g, name)(*args)
    with pytest.raises(TypeError, match="not yet supported"):
        g.predict_with_variance(xs, test_var=0.1)
    for name, args in (("predictive_gradients", (xs,)), ("leave_one_out", ()), ("loo_log_predictive_density", ()),
                       ("predict_with_covariance", (xs,)), ("posterior_samples_f", (xs,))):
        with pytest.raises(TypeError, match="not yet supported"):
            getattr(g, name)(*args)
    # the draw of the inducing rows is SparseGP's
    assert list(BGPLVM(num_inducing=7, seed=3).inducing_draw(50)) == list(cimrgp_amd.SparseGP(num_inducing=7, seed=3).inducing_draw(50))


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_closed_forms_equal_the_gauss_hermite_expectations(d):
    """E[k] and E[k^T k] by a 40^d Gauss-Hermite rule at n = 37, m = 9: measured 1.6e-15 and 2.5e-14 on entries up to 35;
    asserted at 1e-12 relative to the largest entry (the rule converges geometrically for s <= l^2 / 2)."""
    rng = np.random.RandomState(3)
    mu, s, z = rng.randn(37, d), rng.uniform(0, 0.25, (37, d)), rng.randn(9, d)
    s[::5] = 0.0
    ell = [0.8, 1.3][:d]
    g1, g2 = po.gauss_hermite(mu, s, z, ell, 1.4)
    p1, p2 = po.psi1(mu, s, z, ell, 1.4), po.psi2(mu, s, z, ell, 1.4)
    e1, e2 = np.abs(g1 - p1).max() / np.abs(p1).max(), np.abs(g2 - p2).max() / np.abs(p2).max()
    print("gauss-hermite d=%d: psi1 %.2e psi2 %.2e" % (d, e1, e2))
    assert e1 <= 1e-12 and e2 <= 1e-12


@pytest.mark.parametrize("ft", [np.float64, np.longdouble])
def test_limits_and_the_shared_variance_factorisation(ft):
    u = float(np.finfo(ft).eps) / 2
    mu, s, z, _ = po.problem(41, 11, 3, 5)
    ell, sf = [0.8, 1.3, 1.0], 1.4
    k = po.kern(mu, z, ell, sf, ft)
    # s = 0: K_fu and K_uf K_fu
    assert np.abs(po.psi1(mu, 0 * s, z, ell, sf, ft) - k).max() <= 8 * u * sf
    p2 = po.psi2(mu, 0 * s, z, ell, sf, ft)
    # (the exponents of the pairs with the far inducing inputs reach 600: a relative error of a few hundred u each way)
    assert (np.abs(p2 - k.T @ k) <= 5000 * u * (k.T @ k) + 1e-300).all()
    # one variance vector for every row: sf^2 prod (1 + 2 s / l^2)^-1/2 C o (G^T G), exactly
    for sv in (np.array([0.3, 0.0, 2.5]), np.zeros(3), np.array([1e-6, 1e6, 1.0])):
        a, b = po.psi2_shared(mu, sv, z, ell, sf, ft), po.psi2(mu, np.broadcast_to(sv, mu.shape), z, ell, sf, ft)
        assert (np.abs(a - b) <= 2000 * u * np.abs(b) + 1e-300).all()
        assert np.isfinite(np.asarray(a, dtype=np.float64)).all()
    # the pair 40 length-scales apart underflows towards 0 and never becomes NaN
    full = po.psi2(mu, s, z, ell, sf, ft)
    assert np.isfinite(np.asarray(full, dtype=np.float64)).all() and 0 <= full[10, 0] < 1e-150
    # the rounding bounds are those of positive terms: never below the value's own rounding, finite where a term underflows
    for terms, n in ((po.psi2_terms(mu, s, z, ell, sf), 41), (po.psi1_terms(mu, s, z, ell, sf), 1)):
        for dt_u in (2.0 ** -53, 2.0 ** -24):
            b = po.bound(terms[0], terms[1], dt_u, n)
            assert (b >= dt_u * np.asarray(terms[0], dtype=np.float64)).all() and np.isfinite(b).all()


def test_the_bound_at_zero_variance_is_the_vfe_bound():
    mu, s, z, y = po.problem(300, 32, 2, 1, far=False)
    a, b = po.both(mu, 0.0, z, y, 0.9, 1.3, 0.05)
    lml, mean, var = sn.woodbury(mu, z, y, 0, 0.9, 1.3, 0.05, 1e-6, 1, xs=mu[:20])
    # float64 sits ~1e-6 from its own longdouble value on F ~ 450: the two-sided solve of Psi2 by an ill-conditioned K_uu
    print("F(s=0): float64 %.10f longdouble %.10f vfe %.10f" % (float(a.bound), float(b.bound), lml))
    assert abs(float(b.bound) - lml) <= 1e-7 and abs(float(a.bound) - float(b.bound)) <= 1e-4
    assert float(b.kl) == 0.0 and float(b.elbo) == float(b.bound)
    pm, pv = b.predict(mu[:20])
    assert np.abs(np.asarray(pm, dtype=np.float64) - mean).max() <= 1e-7 and np.abs(np.asarray(pv, dtype=np.float64) - var).max() <= 1e-7
    # uncertain test inputs with no variance are exact test inputs
    assert np.abs(b.predict_uncertain(mu[:20], 0.0) - pm).max() <= 1e-15
    # the KL term: 1/2 (s + mu^2 - 1 - log s) per entry with s > 0
    c = po.Model(mu, s, z, y, 0.9, 1.3, 0.05)
    pos = s > 0
    assert abs(float(c.kl) - 0.5 * (s[pos] + mu[pos] ** 2 - 1 - np.log(s[pos])).sum()) <= 1e-9 * float(c.kl)
    assert float(c.elbo) == float(c.bound - c.kl)
