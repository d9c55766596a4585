"""CPU tests of the predictive gradients (include/cimrgp_grad.h): the header's symbols, argument validation without a
GPU, the NumPy restatement of the derivatives against central differences, and the methods that refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

from grad_numpy import block_grad, block_mean_var, central_diff, contract, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grad_header_symbols():
    text = open(os.path.join(ROOT, "include", "cimrgp_grad.h")).read()
    return sorted(set(re.findall(r"^int\s+(cimrgp_\w+)\s*\(", text, re.M)))


def test_grad_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    names = _grad_header_symbols()
    assert names == ["cimrgp_cov_predict_grad", "cimrgp_layer_predict_grad_cov", "cimrgp_trsm_rows_lt",
                     "cimrgp_trsm_rows_lt_batched"]
    assert sorted(_lib.GRAD_SIGNATURES) == names
    for name in names:
        assert hasattr(lib, name), name
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert '#include "cimrgp_grad.h"' in main


def _buf():
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    return buf, (p + 15) // 16 * 16


def test_trsm_rows_lt_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    f = "cimrgp_trsm_rows_lt"
    assert lib.cimrgp_trsm_rows_lt(7, p, 16, 16, p, p, 4, 16, None) < 0 and "dtype" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, None, 16, 16, p, p, 4, 16, None) < 0 and "null pointer" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 16, 16, None, p, 4, 16, None) < 0 and "null pointer" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 0, 16, p, p, 4, 16, None) < 0 and "dimensions" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 16, 16, p, p, -1, 16, None) < 0 and "dimensions" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 16, 8, p, p, 4, 16, None) < 0 and "leading dimension" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 16, 16, p, p, 4, 8, None) < 0 and "leading dimension" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p, 16, 17, p, p, 4, 16, None) < 0 and "16 bytes" in _lib.last_error()
    assert lib.cimrgp_trsm_rows_lt(_lib.F64, p + 8, 16, 16, p, p, 4, 16, None) < 0 and "aligned" in _lib.last_error()
    assert f in _lib.last_error()
    ws = int(lib.cimrgp_potrf_workspace_bytes(_lib.F64, 16))
    rc = lib.cimrgp_trsm_rows_lt_batched(_lib.F64, p, 16, 16, 256, p, ws // 2, p, 4, 16, 64, 2, None)
    assert rc < 0 and "workspace stride" in _lib.last_error()
    rc = lib.cimrgp_trsm_rows_lt_batched(_lib.F64, p, 16, 16, 256, p, ws, p, 4, 16, 32, 2, None)
    assert rc < 0 and "stride too small" in _lib.last_error()
    rc = lib.cimrgp_trsm_rows_lt_batched(_lib.F64, p, 16, 16, 256, p, ws, p, 4, 16, 64, 0, None)
    assert rc < 0 and "batch" in _lib.last_error()


def test_cov_predict_grad_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    args = dict(dtype=_lib.F64, cov=_lib.COV_RBF, x=p, n=16, d=2, alpha=p, q=2, xs=p, ns=4, ell=1.0, sf2=1.0, beta=p, ldb=16,
                mg=p, vg=p)

    def call(**kw):
        a = dict(args, **kw)
        return lib.cimrgp_cov_predict_grad(a["dtype"], a["cov"], a["x"], a["n"], a["d"], a["alpha"], a["q"], a["xs"], a["ns"],
                                           a["ell"], a["sf2"], a["beta"], a["ldb"], a["mg"], a["vg"], 0, None)
    assert call(dtype=3) < 0 and "cimrgp_cov_predict_grad" in _lib.last_error() and "dtype" in _lib.last_error()
    assert call(cov=4) < 0 and "unknown covariance" in _lib.last_error()
    assert call(cov=-1) < 0 and "unknown covariance" in _lib.last_error()
    assert call(n=0) < 0 and "dimensions" in _lib.last_error()
    assert call(d=0) < 0 and "input dimension" in _lib.last_error()
    assert call(d=9) < 0 and "input dimension" in _lib.last_error()
    assert call(q=0) < 0 and "outputs" in _lib.last_error()
    assert call(q=9) < 0 and "outputs" in _lib.last_error()
    assert call(x=None) < 0 and "null pointer" in _lib.last_error()
    assert call(alpha=None) < 0 and "alpha" in _lib.last_error()
    assert call(beta=None) < 0 and "beta" in _lib.last_error()
    assert call(ldb=15) < 0 and "leading dimension" in _lib.last_error()
    assert call(ell=0.0) < 0 and "positive" in _lib.last_error()
    # what is not needed is not required: no variance output, no beta
    assert call(vg=None, beta=None, ldb=0, ns=0) == 0


def test_layer_predict_grad_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    ws = int(lib.cimrgp_potrf_workspace_bytes(_lib.F64, 16))
    args = dict(dtype=_lib.F64, cov=_lib.COV_MATERN32, n=16, d=1, ns=8, batch=1, q=2, ldl=16, ldw=16, alpha=p, w=p, l=p)

    def call(**kw):
        a = dict(args, **kw)
        return lib.cimrgp_layer_predict_grad_cov(a["dtype"], a["cov"], p, p, a["n"], a["d"], p, p, a["ns"], a["batch"], 1.0, 1.0,
                                                 a["l"], a["ldl"], 256, p, ws, a["alpha"], a["q"], a["w"], a["ldw"], 128, p, p, 1,
                                                 None)
    assert call(dtype=2) < 0 and "cimrgp_layer_predict_grad_cov" in _lib.last_error() and "dtype" in _lib.last_error()
    assert call(cov=9) < 0 and "unknown covariance" in _lib.last_error()
    assert call(n=0) < 0 and "dimensions" in _lib.last_error()
    assert call(d=0) < 0 and "input dimension" in _lib.last_error()
    assert call(q=0) < 0 and "outputs" in _lib.last_error()
    assert call(q=9) < 0 and "outputs" in _lib.last_error()
    assert call(batch=0) < 0 and "batch" in _lib.last_error()
    assert call(alpha=None) < 0 and "null pointer" in _lib.last_error()
    assert call(w=None) < 0 and "null pointer" in _lib.last_error()
    assert call(l=None) < 0 and "null pointer" in _lib.last_error()
    assert call(ldl=8) < 0 and "leading dimension" in _lib.last_error()
    assert call(ldw=8) < 0 and "leading dimension" in _lib.last_error()
    assert call(ldw=17) < 0 and "16 bytes" in _lib.last_error()


@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_numpy_gradients_match_central_differences(cov, d):
    """The table of g(r) (include/cimrgp_grad.h) against central differences of the NumPy predictive mean and
    variance."""
    rng = np.random.default_rng(10 * cov + d)
    n, ns, q = 40, 12, 3
    x = rng.uniform(-1, 1, size=(n, d))
    r = rng.normal(size=(n, q))
    xs = rng.uniform(-1, 1, size=(ns, d))
    ell, sf2, noise = 0.6, 1.4, 0.05
    mg, vg = block_grad(x, r, xs, cov, ell, sf2, noise)
    dm, dv = central_diff(lambda t: block_mean_var(x, r, t, cov, ell, sf2, noise), xs, 1e-6)
    assert rel(mg, dm) < 1e-6
    assert rel(vg, dv) < 1e-6
    # the contraction with the mean only gives the same mean gradient
    K = np.eye(n)
    mg2, vg2 = contract(x, np.linalg.solve(K, r), xs, cov, ell, sf2)
    assert vg2 is None and mg2.shape == (ns, d, q)


def test_matern12_gradient_is_zero_at_a_training_point():
    x = np.array([[0.0], [0.5], [1.0]])
    alpha = np.ones((3, 1))
    mg, _ = contract(x, alpha, x[:1].copy(), 1, 1.0, 1.0)
    # only the two other points contribute; the pair at r = 0 follows GPy's convention (0)
    want = -(np.exp(-0.5) / 0.5 * (0.0 - 0.5) + np.exp(-1.0) / 1.0 * (0.0 - 1.0))
    assert np.isfinite(mg).all() and abs(mg[0, 0, 0] - want) < 1e-15


def test_predictive_gradients_refuse_what_is_not_built():
    from cimrgp_amd.MRGP import MultiResolutionGaussianProcess
    from cimrgp_amd.ReducedRank import ReducedRankMRGP
    m = object.__new__(MultiResolutionGaussianProcess)
    m.adaptive_inputs = True
    with pytest.raises(TypeError, match="not yet supported"):
        m.predictive_gradients(np.zeros((4, 1)))
    rr = object.__new__(ReducedRankMRGP)
    with pytest.raises(TypeError, match="not yet supported"):
        rr.predictive_gradients(np.zeros((4, 1)))


def test_predictive_gradients_check_the_index_set_like_get_predicted_mean():
    import cimrgp_amd as ca
    m = object.__new__(MultiResolutionGaussianProcess_())
    m.adaptive_inputs = False
    m.index_set_obj = ca.IndexSetUniform(256, 2, 2)
    m.n_regions = [len(b) for b in m.index_set_obj.bounds]
    xs = np.zeros((64, 1))
    for bad, nr in ((ca.IndexSetUniform(64, 3, 2), None), (ca.IndexSetUniform(64, 2, 4), None),
                    (ca.IndexSetUniform(64, 2, 2), [1, 2, 3])):
        with pytest.raises(ValueError) as ref:
            m.get_predicted_mean(xs, bad, nr)
        with pytest.raises(ValueError) as got:
            m.predictive_gradients(xs, bad, nr)
        assert str(got.value) == str(ref.value)


def MultiResolutionGaussianProcess_():
    from cimrgp_amd.MRGP import MultiResolutionGaussianProcess
    return MultiResolutionGaussianProcess
