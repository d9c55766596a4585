"""CPU tests of the inducing-point sparse GP (include/cimrgp_sparse.h): the header's symbols, the scratch formula, the
two NumPy forms against each other and against the exact GP, the documented draw of inducing inputs, and what the
plugin refuses without a GPU."""
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import sparse_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: (n, m, d, cov, ell): the acceptance inputs (sf = 1, noise = 0.01, eps = 1e-6); the GPU tests add n = 20 000
SETS = [(1500, 128, 1, 0, 0.3), (1500, 200, 2, 0, 0.5), (1500, 128, 2, 0, 1.0), (1500, 200, 2, 2, 1.0)]
SF, NOISE, EPS = 1.0, 0.01, 1e-6


def test_sparse_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_sparse_lambda", "cimrgp_sparse_tail", "cimrgp_wsyrk_tn", "cimrgp_wsyrk_tn_scratch_bytes"]
    assert sorted(_lib.SPARSE_SIGNATURES) == names
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SPARSE_SIGNATURES[name][1], name
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert '#include "cimrgp_sparse.h"' in main
    assert int(re.search(r"#define CIMRGP_WSYRK_MAX_M (\d+)", text).group(1)) >= 4096
    assert eval(re.search(r"#define CIMRGP_WSYRK_MAX_N (\(.*\))", text).group(1)) >= 1 << 20


@pytest.mark.parametrize("dtype,esz", [(_lib.F64, 8), (_lib.F32, 4)])
def test_wsyrk_scratch_bytes_by_formula(dtype, esz):
    lib = _lib.load()
    for n, m, q in ((1, 16, 0), (255, 100, 2), (4097, 1000, 2), (65536, 1024, 2), (30001, 2048, 8), (8192, 4096, 1),
                    (262144, 1000, 1), (1 << 20, 4096, 8), (1 << 24, 16384, 0)):
        assert int(lib.cimrgp_wsyrk_tn_scratch_bytes(dtype, n, m, q)) == sn.scratch_bytes(esz, n, m, q), (n, m, q)
    for bad in ((0, 16, 0), (16, 0, 0), ((1 << 24) + 1, 16, 0), (16, 16385, 0), (16, 16, 9), (16, 16, -1)):
        assert int(lib.cimrgp_wsyrk_tn_scratch_bytes(dtype, *bad)) == 0, bad
    assert int(lib.cimrgp_wsyrk_tn_scratch_bytes(7, 100, 100, 1)) == 0
    # the split fills the machine where there is K to cut: 36 tiles x 28 slices at m = 1024
    assert sn.slices(65536, 1024) == (28, 2368) and sn.slices(255, 100) == (1, 256) and sn.slices(8192, 4096)[0] == 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m,d,cov,ell", SETS)
def test_woodbury_and_dense_forms_agree(n, m, d, cov, ell, mode):
    """Both forms are backward stable in K_uu + eps sf I, whose condition number is at most (m sf + eps sf) / (eps sf):
    they differ by at most a small multiple of u m / eps = 1.1e-16 x 200 / 1e-6 = 2.2e-8 (observed: some 1e-10)."""
    x, z, r, xs = sn.problem(n, m, d, seed=n + m + d + cov)
    lw, mw, vw = sn.woodbury(x, z, r, cov, ell, SF, NOISE, EPS, mode, xs)
    ld, md, vd = sn.dense(x, z, r, cov, ell, SF, NOISE, EPS, mode, xs)
    bar = 1.1e-16 * m / EPS
    print(abs(lw - ld) / abs(ld), np.abs(mw - md).max(), np.abs(vw - vd).max())
    assert abs(lw - ld) <= bar * abs(ld)
    assert np.abs(mw - md).max() <= bar
    assert np.abs(vw - vd).max() <= bar
    assert (vw > -bar).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [1, 2])
def test_inducing_at_the_data_is_the_exact_gp(d, mode):
    """Z = X, eps = 0: Q_ff = K_ff, lambda = noise and the trace term is 0, so FITC and VFE are the exact GP (Matern 1/2:
    K_ff is well conditioned).  CPU-only identity, bar 1e-10."""
    rng = np.random.default_rng(d)
    n = 256
    x = rng.uniform(-2, 2, size=(n, d))
    r = np.stack([np.sin(2 * x).sum(axis=1), np.cos(x).prod(axis=1)], axis=1) + 0.1 * rng.normal(size=(n, 2))
    xs = rng.uniform(-2.2, 2.2, size=(100, d))
    ls, ms, vs = sn.woodbury(x, x, r, 1, 1.0, SF, NOISE, 0.0, mode, xs)
    le, me, ve = sn.exact(x, r, 1, 1.0, SF, NOISE, xs)
    assert abs(ls - le) <= 1e-10 * abs(le)
    assert np.abs(ms - me).max() <= 1e-10
    assert np.abs(vs - ve).max() <= 1e-10


def test_the_draw_of_inducing_inputs_is_the_documented_permutation():
    from cimrgp_amd import SGP_FITC, SparseGP, SparseGP_RBF
    assert (SGP_FITC.name, SparseGP_RBF.name) == ('SGP_FITC', 'SparseGP_RBF')
    assert (SGP_FITC().approximation, SparseGP_RBF().approximation, SparseGP().approximation) == ('fitc', 'vfe', 'fitc')
    assert SGP_FITC().num_inducing == 1000 and SGP_FITC().optimize is False
    g = SGP_FITC(num_inducing=50, seed=3)
    x = np.random.default_rng(0).normal(size=(400, 2))
    g.data_mean, g.data_std = x.mean(axis=0), x.std(axis=0)
    ids = np.random.RandomState(3).permutation(400)[:50]
    assert np.array_equal(g._inducing_inputs(x), x[ids]) and np.array_equal(g.inducing_ids, ids)
    assert np.array_equal(SGP_FITC(num_inducing=1000, seed=1).inducing_draw(30), np.random.RandomState(1).permutation(30))
    # a given Z is in the caller's units: z-scored with the inputs
    zc = np.array([[1.0, 2.0], [3.0, -1.0]])
    gz = SGP_FITC(Z=zc)
    gz.data_mean, gz.data_std = g.data_mean, g.data_std
    assert np.allclose(gz._inducing_inputs(x), (zc - g.data_mean) / g.data_std) and gz.inducing_ids is None


def test_sparse_plugin_refuses_bad_arguments():
    from cimrgp_amd import SGP_FITC, SparseGP
    with pytest.raises(ValueError, match="approximation"):
        SparseGP(approximation='svgp')
    with pytest.raises(ValueError, match="nu"):
        SGP_FITC(nu=2.0)
    with pytest.raises(ValueError, match="num_inducing"):
        SGP_FITC(num_inducing=0)
    for f in (lambda g: g.predict(np.zeros((2, 1))), lambda g: g.log_marginal_likelihood()):
        g = SGP_FITC()
        g.preprocess = False
        with pytest.raises(RuntimeError, match="fit"):
            f(g)
