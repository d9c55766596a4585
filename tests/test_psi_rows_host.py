"""CPU tests of the predictive variance at uncertain test inputs (include/cimrgp_psi_rows.h; DESIGN.md, "Predictive
variance at uncertain test inputs"): the header's symbols, every refusal of the entry point that precedes a HIP call, the
scratch size against its Python restatement, the oracle of tests/psi_rows_numpy.py against a Gauss-Hermite evaluation of
the law of total variance and against ``Model.predict`` at zero variance, and the argument checks of
``UncertainInputBlock.predict_moments`` and ``BayesianGPLVM.predict_uncertain`` beside the refusals that stay."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import psi_grad_numpy as pg
import psi_numpy as po
import psi_rows_numpy as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
QUAD = 'cimrgp_psi2_rows_quad'


# ---- the header -------------------------------------------------------------------------------------------------------
def test_psi_rows_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_psi_rows.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == [QUAD, QUAD + "_scratch_bytes"]
    assert sorted(_lib.PSI_ROWS_SIGNATURES) == names and _lib.HEADERS["cimrgp_psi_rows.h"] is _lib.PSI_ROWS_SIGNATURES
    for name in names:
        assert getattr(lib, name).argtypes == _lib.PSI_ROWS_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.PSI_ROWS_SIGNATURES[name][0], name
    order = list(_lib.HEADERS)
    assert order[-1] == "cimrgp_svgp.h" and order.index("cimrgp_psi_rows.h") == order.index("cimrgp_psi_grad.h") + 1
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert main.index('#include "cimrgp_psi_grad.h"') < main.index('#include "cimrgp_psi_rows.h"') < main.index('#include "cimrgp_svgp.h"')
    assert " psi_rows " in open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    assert int(re.search(r"#define CIMRGP_PSI_ROWS_GROUPS (\d+)", text).group(1)) == _lib.PSI_ROWS_GROUPS == pr.GROUPS


# ---- refusals --------------------------------------------------------------------------------------------------------
BASE = [('dtype', 1), ('mu', 'P'), ('s', 'P'), ('z', 'P'), ('n', 600), ('m', 100), ('d', 2), ('ell', 'P'), ('sf2', 1.3), ('c', 'P'),
        ('ldc', 112), ('a', 'P'), ('lda', 3), ('q', 3), ('tr', 'P'), ('quad', 'P'), ('ldq', 3), ('scratch', 'P'), ('scratch_bytes', 1 << 40),
        ('bad', 'P'), ('stream', None)]
POINTERS = ['mu', 's', 'z', 'ell', 'c', 'a', 'tr', 'quad', 'scratch', 'bad']
ROWS = ([({'dtype': 7}, 'unknown dtype')] + [({p: None}, 'null pointer') for p in POINTERS] + [
    ({'n': 0}, 'n must be in [1, 16777216]'), ({'n': (1 << 24) + 1}, 'n must be in [1, 16777216]'),
    ({'m': 0}, 'm must be in [1, 16384]'), ({'m': 16385, 'ldc': 16400}, 'm must be in [1, 16384]'),
    ({'d': 0}, 'input dimension must be in [1, 8]'), ({'d': 9}, 'input dimension must be in [1, 8]'),
    ({'q': 0}, 'the number of outputs must be in [1, 8]'), ({'q': 9, 'lda': 9, 'ldq': 9}, 'the number of outputs must be in [1, 8]'),
    ({'sf2': 0.0}, 'sf2 must be positive'), ({'sf2': -1.0}, 'sf2 must be positive'), ({'sf2': float('nan')}, 'sf2 must be positive'),
    ({'ldc': 99}, 'leading dimension too small'), ({'lda': 2}, 'leading dimension too small'), ({'ldq': 2}, 'leading dimension too small'),
    ({'scratch': 'P+8'}, 'scratch must be 16-byte aligned'),
    ({'scratch_bytes': 'one short'}, 'scratch too small'), ({'scratch_bytes': 0}, 'scratch too small'),
    ({'dtype': 7, 'mu': None, 'n': 0, 'd': 0, 'q': 0}, 'unknown dtype')])


def test_psi_rows_refusals_status_and_text():
    """Every refusal returns -1 with its text in the call's name; the operands stand on 512 bytes of host memory, so a check
    that came after a launch would not return at all."""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    stand_in = {"P": p, "P+8": p + 8, "one short": lib.cimrgp_psi2_rows_quad_scratch_bytes(1, 600, 100, 2, 3) - 1}
    assert stand_in["one short"] > 0 and len(BASE) == len(_lib.PSI_ROWS_SIGNATURES[QUAD][1])
    for broken, text in ROWS:
        assert broken and set(broken) <= {k for k, _ in BASE}, broken
        args = [broken.get(k, v) for k, v in BASE]
        rc = getattr(lib, QUAD)(*[stand_in.get(a, a) if isinstance(a, str) else a for a in args])
        print(broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (-1, '%s: %s' % (QUAD, text)), broken


def test_every_check_of_the_entry_point_has_a_row():
    src = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "psi_rows.hip")).read()
    ext = src[src.index('extern "C" {'):]
    body = ext[ext.index("int %s(" % QUAD):]
    body = body[:body.index("\n}\n")]
    checks = re.findall(r'CIMRGP_REQUIRE\(.*?, fn,\s*"([^"]+)"\);', body, re.S)
    assert len(checks) == 10
    assert set(checks) == {text for _, text in ROWS}
    assert body.rindex("CIMRGP_REQUIRE") < body.index("with_dtype(")        # every check stands before the first launch


def test_scratch_bytes_and_groups_are_the_python_restatement():
    lib = _lib.load()
    for n, m in ((1, 1), (63, 64), (64, 65), (150, 40), (300, 65), (257, 130), (64, 321), (4097, 100), (65536, 1000), (1 << 24, 16384),
                 (1 << 24, 1)):
        for dtype, esz in ((0, 4), (1, 8)):
            for d, q in ((1, 1), (2, 3), (8, 8)):
                got = lib.cimrgp_psi2_rows_quad_scratch_bytes(dtype, n, m, d, q)
                assert got == pr.scratch_bytes(esz, n, m, d, q) and got % 16 == 0 and got > 0, (n, m, d, q, dtype)
    for bad in ((7, 10, 10, 2, 1), (1, 0, 10, 2, 1), (1, 10, 0, 2, 1), (1, 10, 10, 0, 1), (1, 10, 10, 9, 1), (1, 10, 10, 2, 0), (1, 10, 10, 2, 9),
                (1, (1 << 24) + 1, 10, 2, 1), (1, 10, 16385, 2, 1)):
        assert lib.cimrgp_psi2_rows_quad_scratch_bytes(*bad) == 0, bad
    # the groups: one tile per group up to 16 tiles, never more than 16 groups, every tile in exactly one group
    assert pr.group_rule(1) == (1, 1, 1) and pr.group_rule(130) == (6, 1, 6) and pr.group_rule(321) == (11, 2, 21)
    assert pr.group_rule(1000) == (16, 9, 136) and pr.group_rule(16384) == (16, 2056, 32896)
    for m in range(1, 16385, 61):
        groups, per, tiles = pr.group_rule(m)
        assert 1 <= groups <= pr.GROUPS and (groups - 1) * per < tiles <= groups * per, m
    # a (row, group) subtotal per output is all the call keeps per row: well under 100 MB at the flagship size, q = 8
    assert lib.cimrgp_psi2_rows_quad_scratch_bytes(1, 65536, 1000, 2, 8) < 100e6


# ---- the oracle --------------------------------------------------------------------------------------------------------
def _model(d, ft, seed=0):
    n, m, q = (80, 16, 2) if d == 1 else (60, 12, 2)
    mu, s, z, y = po.problem(n, m, d, 40 + d + seed, q=q, far=False)
    s = np.minimum(s, 2.0)
    ell = np.array([0.9, 1.4][:d])
    return po.Model(mu, s, z, y, ell, 1.3, 0.3, ft=ft), n


def _test_inputs(d, ns):
    xs = np.random.RandomState(5).randn(ns, d)
    xs_var = 10.0 ** np.random.RandomState(6).uniform(-3, 0, size=(ns, d))
    xs_var[::4] = 0.0
    return xs, xs_var


@pytest.mark.parametrize("d", [1, 2])
def test_oracle_moments_equal_the_gauss_hermite_law_of_total_variance(d):
    """The closed form against a 60^d Gauss-Hermite rule over ``Model.predict`` in longdouble, variances from three decades
    with every fourth row exactly 0: 1e-9 absolute on variances of 0.01 .. 1 (the rule itself converges to about 1e-11)."""
    model, _ = _model(d, LD)
    xs, xs_var = _test_inputs(d, 12 if d == 2 else 24)
    mean, var = pr.moments(model, xs, xs_var)
    gmean, gvar = pr.moments_gauss_hermite(model, xs, xs_var, nodes=60)
    em, ev = float(np.abs(mean - gmean).max()), float(np.abs(var - gvar).max())
    print("d = %d: |mean - GH| %.2e, |var - GH| %.2e on variances %.3g .. %.3g" % (d, em, ev, float(var.min()), float(var.max())))
    assert var.shape == gvar.shape == (xs.shape[0], 2) and (var > 0).all()
    assert em <= 1e-9 and ev <= 1e-9
    # the second part, the spread of the posterior mean over the input, is there and differs from column to column
    spread = var - (model.sf - pr.rows_quad(xs, xs_var, model.z, model.ell, model.sf, *pr.weights(model), ft=LD)['tr'])[:, None]
    assert (spread > -1e-14).all() and float(spread.max()) > 1e-4 and float(np.abs(spread[:, 0] - spread[:, 1]).max()) > 1e-6


@pytest.mark.parametrize("d", [1, 2, 3])
def test_oracle_moments_at_zero_variance_are_model_predict(d):
    """xs_var = 0: the mean is ``Model.predict``'s and every column of the variance its variance; ``include_noise`` adds the noise."""
    rng = np.random.RandomState(3)
    mu, s, z, y = po.problem(50, 10, d, 9 + d, q=3, far=False)
    model = po.Model(mu, s, z, y, np.array([0.9, 1.4, 1.1][:d]), 1.3, 0.3, ft=LD)
    xs = rng.randn(20, d)
    want_mean, want_var = model.predict(xs)
    for zero in (0.0, np.zeros(d), np.zeros((20, d))):
        mean, var = pr.moments(model, xs, zero)
        assert float(np.abs(mean - want_mean).max()) <= 1e-14
        assert var.shape == (20, 3) and float(np.abs(var - want_var[:, None]).max()) <= 1e-11
    noisy = pr.moments(model, xs, 0.0, include_noise=True)[1]
    assert float(np.abs(noisy - var - model.noise).max()) <= 1e-15


def test_the_rounding_bound_is_finite_and_covers_the_stored_value():
    mu, s, z, _ = po.problem(41, 11, 3, 5)
    ell, sf = [0.8, 1.3, 1.0], 1.4
    rng = np.random.RandomState(2)
    c, a = rng.randn(11, 11), rng.randn(11, 3)
    c = c + c.T
    val, wts = pr.rows_quad(mu, s, z, ell, sf, c, a, LD), pr.rows_quad(mu, s, z, ell, sf, c, a, LD, bound=True)
    full = po.psi2(mu[:1], s[:1], z, ell, sf, LD)                     # one row's Psi2 is psi2 of that row alone
    assert abs(val['tr'][0] - (c * full).sum()) <= 1e-15 * np.abs(c * full).sum()
    assert float(np.abs(val['quad'][0] - np.einsum('jc,jk,kc->c', a, full, a)).max()) <= 1e-15 * float((np.abs(a).sum(axis=0) ** 2).max()) * sf ** 2
    for key in ("tr", "quad"):
        for u in (2.0 ** -53, 2.0 ** -24):
            b = pg.grad_bound(val[key], wts[key], u)
            assert b.shape == np.shape(val[key]) and np.isfinite(b).all(), key
            assert (b >= u * np.abs(np.asarray(val[key], dtype=np.float64))).all() and (b > 0).all(), key


# ---- the block and the plugin ------------------------------------------------------------------------------------------
def test_block_argument_checks_and_the_refusals_that_stay():
    torch = pytest.importorskip("torch")
    from cimrgp_amd import UncertainInputBlock
    from cimrgp_amd.KernelClass import RBFKernel
    f64 = torch.float64
    mu = torch.arange(30, dtype=f64).reshape(10, 3) / 10
    z = torch.zeros((4, 3), dtype=f64)
    blk = UncertainInputBlock(mu, 0.1, z, RBFKernel(l=0.7, sf=1.3, noise=0.5))
    xs = torch.zeros((5, 3), dtype=f64)
    mean, var = torch.empty((5, 2), dtype=f64), torch.empty((5, 2), dtype=f64)
    for xs_var in (0.1, [0.1, 0.0, 0.2], torch.full((5, 3), 0.1, dtype=f64)):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before predict_moments"):
            blk.predict_moments(xs, xs_var, mean, var)
    for wrong in ([0.1, 0.2], torch.full((4, 3), 0.1, dtype=f64), torch.full((5, 2), 0.1, dtype=f64), -0.1, float('nan'),
                  torch.full((5, 3), 0.1, dtype=torch.float32)):
        with pytest.raises(ValueError, match="x_var"):
            blk.predict_moments(xs, wrong, mean, var)
    # the variance through predict() stays refused, fitted or not: it is (ns, q) and has its own method
    with pytest.raises(TypeError, match="not yet supported"):
        blk.predict(xs, mean, torch.empty(5, dtype=f64), xs_var=0.1)


def test_plugin_argument_checks_and_the_refusals_that_stay():
    import inspect
    from cimrgp_amd import BGPLVM
    from cimrgp_amd.GPLVM import BayesianGPLVM
    assert not hasattr(BGPLVM, 'predict_uncertain') and not hasattr(BGPLVM, 'predict_moments')
    sig = inspect.signature(BayesianGPLVM.predict_uncertain).parameters
    assert list(sig) == ['self', 'test_data', 'test_var', 'include_noise', 'budget_bytes']
    assert sig['include_noise'].default is False and sig['budget_bytes'].default is None
    xs = np.zeros((3, 2))
    g = BayesianGPLVM()
    for tv in (0.1, [0.1, 0.2], np.full((3, 2), 0.1)):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before predict_uncertain"):
            g.predict_uncertain(xs, tv)
    for plugin in (g, BGPLVM()):
        with pytest.raises(TypeError, match="not yet supported"):
            plugin.predict_with_variance(xs, test_var=0.1)
