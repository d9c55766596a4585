"""CPU tests of the leave-one-out cross-validation (include/cimrgp_loo.h): the header's symbols, argument validation
without a GPU, the scratch formula, the NumPy restatement against brute-force refits, and the methods that refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

from loo_numpy import kcov, kinv_diag, loo_brute_force, loo_closed_form, rel, scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loo_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_loo.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_kinv_diag", "cimrgp_kinv_diag_batched", "cimrgp_kinv_diag_scratch_bytes", "cimrgp_loo",
                     "cimrgp_loo_batched", "cimrgp_trtri_rows"]
    assert sorted(_lib.LOO_SIGNATURES) == names
    for name in names:
        assert hasattr(lib, name), name
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert '#include "cimrgp_loo.h"' in main


def _buf():
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    return buf, (p + 15) // 16 * 16


def _err():
    return _lib.last_error()


def test_trtri_rows_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    f = lib.cimrgp_trtri_rows
    ok = dict(dtype=_lib.F64, l=p, n=600, ldl=608, ws=p, r0=256, m=100, u=p, ldu=608)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["dtype"], a["l"], a["n"], a["ldl"], a["ws"], a["r0"], a["m"], a["u"], a["ldu"], None)
    assert call(dtype=5) < 0 and "dtype" in _err() and "cimrgp_trtri_rows" in _err()
    for k in ("l", "ws", "u"):
        assert call(**{k: None}) < 0 and "null pointer" in _err() and "cimrgp_trtri_rows" in _err()
    assert call(n=0) < 0 and "dimensions" in _err()
    assert call(m=-1) < 0 and "dimensions" in _err()
    assert call(r0=100) < 0 and "multiple of 256" in _err() and "cimrgp_trtri_rows" in _err()
    assert call(r0=-256) < 0 and "multiple of 256" in _err()
    assert call(r0=512, m=100) < 0 and "must lie in" in _err()
    assert call(r0=768, m=0) < 0 and "must lie in" in _err()
    assert call(ldl=592) < 0 and "leading dimension" in _err()
    assert call(ldu=592) < 0 and "leading dimension" in _err()
    assert call(ldu=609) < 0 and "16 bytes" in _err()
    assert call(ldl=609) < 0 and "16 bytes" in _err()
    assert call(u=p + 8) < 0 and "aligned" in _err() and "cimrgp_trtri_rows" in _err()
    assert call(dtype=_lib.F32, ldu=602) < 0 and "16 bytes" in _err()
    assert call(m=0) == 0            # nothing to do: no device work


def test_kinv_diag_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    need = int(lib.cimrgp_kinv_diag_scratch_bytes(_lib.F64, 600, 256))
    ok = dict(dtype=_lib.F64, l=p, n=600, ldl=608, ws=p, scratch=p, nbytes=need, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cimrgp_kinv_diag(a["dtype"], a["l"], a["n"], a["ldl"], a["ws"], a["scratch"], a["nbytes"], a["out"], None)
    assert call(dtype=-1) < 0 and "dtype" in _err() and "cimrgp_kinv_diag" in _err()
    for k in ("l", "ws", "scratch", "out"):
        assert call(**{k: None}) < 0 and "null pointer" in _err()
    assert call(n=0) < 0 and "dimensions" in _err()
    assert call(ldl=599) < 0 and "leading dimension" in _err()
    assert call(ldl=601) < 0 and "16 bytes" in _err()
    assert call(scratch=p + 8) < 0 and "aligned" in _err()
    assert call(nbytes=need - 1) < 0 and "scratch too small" in _err() and "cimrgp_kinv_diag" in _err()
    assert "batched" not in _err()
    ws = int(lib.cimrgp_potrf_workspace_bytes(_lib.F64, 600))
    okb = dict(ok, l_stride=600 * 608, ws_stride=ws, nbytes=3 * need, batch=3)

    def callb(**kw):
        a = dict(okb, **kw)
        return lib.cimrgp_kinv_diag_batched(a["dtype"], a["l"], a["n"], a["ldl"], a["l_stride"], a["ws"], a["ws_stride"],
                                            a["scratch"], a["nbytes"], a["out"], a["batch"], None)
    assert callb(batch=0) < 0 and "batch" in _err() and "cimrgp_kinv_diag_batched" in _err()
    assert callb(batch=70000) < 0 and "batch" in _err()
    assert callb(dtype=9) < 0 and "dtype" in _err()
    assert callb(out=None) < 0 and "null pointer" in _err()
    assert callb(ws_stride=ws // 2) < 0 and "workspace stride" in _err()
    assert callb(ws_stride=ws + 8) < 0 and "16 bytes" in _err()
    assert callb(l_stride=600 * 300) < 0 and "stride too small" in _err()
    assert callb(l_stride=600 * 608 + 1) < 0 and "16 bytes" in _err()
    assert callb(nbytes=3 * need - 1) < 0 and "scratch too small" in _err() and "cimrgp_kinv_diag_batched" in _err()


def test_loo_tail_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    f = lib.cimrgp_loo
    assert f(4, p, p, p, 10, 2, p, p, None) < 0 and "dtype" in _err() and "cimrgp_loo" in _err()
    assert f(_lib.F64, p, p, None, 10, 2, p, p, None) < 0 and "null pointer" in _err()
    assert f(_lib.F64, None, p, p, 10, 2, p, p, None) < 0 and "null pointer" in _err()
    assert f(_lib.F64, p, None, p, 10, 2, p, p, None) < 0 and "null pointer" in _err()
    assert f(_lib.F64, p, p, p, -1, 2, p, p, None) < 0 and "dimensions" in _err()
    assert f(_lib.F64, p, p, p, 10, 0, p, p, None) < 0 and "outputs" in _err()
    assert f(_lib.F64, p, p, p, 10, 9, p, p, None) < 0 and "outputs" in _err() and "batched" not in _err()
    # what is not needed is not required; no output, no work
    assert f(_lib.F64, None, None, p, 10, 2, None, None, None) == 0
    g = lib.cimrgp_loo_batched
    assert g(_lib.F64, p, None, p, p, 10, 2, 2, p, p, None) < 0 and "starts" in _err() and "cimrgp_loo_batched" in _err()
    assert g(_lib.F64, p, p, p, p, 10, 2, 0, p, p, None) < 0 and "batch" in _err()
    assert g(_lib.F64, p, p, p, p, 10, 9, 2, p, p, None) < 0 and "outputs" in _err() and "cimrgp_loo_batched" in _err()
    assert g(6, p, p, p, p, 10, 2, 2, p, p, None) < 0 and "dtype" in _err()


@pytest.mark.parametrize("dtype,esz", [(_lib.F64, 8), (_lib.F32, 4)])
def test_kinv_diag_scratch_bytes_by_formula(dtype, esz):
    lib = _lib.load()
    for n, strip in ((1, 1), (255, 256), (600, 0), (600, 257), (600, 100000), (4096, 1024), (5000, 1000), (65536, 4096)):
        assert int(lib.cimrgp_kinv_diag_scratch_bytes(dtype, n, strip)) == scratch_bytes(esz, n, strip), (n, strip)
    assert int(lib.cimrgp_kinv_diag_scratch_bytes(dtype, 0, 256)) == 0
    assert int(lib.cimrgp_kinv_diag_scratch_bytes(3, 100, 256)) == 0
    assert scratch_bytes(8, 600, 0) == 256 * 608 * 8


@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_numpy_loo_matches_brute_force_refits(cov, d):
    """y_i - alpha_i / [K^-1]_ii and 1 / [K^-1]_ii against deleting point i and solving again."""
    rng = np.random.default_rng(100 * cov + d)
    n, q = 96, 3
    x = rng.uniform(-1, 1, size=(n, d))
    sf2 = 1.3
    K = kcov(x, x, cov, 0.5, sf2) + 1e-2 * sf2 * np.eye(n)
    y = rng.normal(size=(n, q))
    r = y - (0.3 * rng.normal(size=(n, q)) + rng.normal(size=(1, q)))          # y - f_bar - bias
    mean, var = loo_closed_form(K, y, r)
    bmean, bvar = loo_brute_force(K, y, r)
    assert rel(mean, bmean) < 1e-10
    assert rel(var, bvar) < 1e-10
    assert rel(kinv_diag(np.linalg.cholesky(K)), np.diag(np.linalg.inv(K))) < 1e-10


def test_leave_one_out_refuses_what_is_not_built():
    from cimrgp_amd.MRGP import MultiResolutionGaussianProcess
    from cimrgp_amd.ReducedRank import ReducedRankMRGP
    from cimrgp_amd.Posteriors import DenseBlock
    from cimrgp_amd.RegressionInput import GP_RBF, GP_Matern
    m = object.__new__(MultiResolutionGaussianProcess)
    m._fitted, m.keep_factors, m.n_layers = False, True, 3
    for f in (m.leave_one_out, m.get_loo_likelihood):
        with pytest.raises(RuntimeError, match="fit"):
            f()
    m._fitted, m.keep_factors = True, False
    for f in (m.leave_one_out, m.get_loo_likelihood):
        with pytest.raises(RuntimeError, match="keep_factors=True"):
            f()
    m.keep_factors = True
    for bad in (3, -1, 17):
        with pytest.raises(ValueError, match="layer"):
            m.leave_one_out(bad)
        with pytest.raises(ValueError, match="layer"):
            m.get_loo_likelihood(layer=bad)
    rr = object.__new__(ReducedRankMRGP)
    for f in (rr.leave_one_out, rr.get_loo_likelihood):
        with pytest.raises(TypeError, match="not yet supported"):
            f()
    blk = object.__new__(DenseBlock)
    blk.lbuf = None
    with pytest.raises(RuntimeError, match="keep_factors=True"):
        blk.loo(None, None, None)
    for g in (GP_RBF(), GP_Matern(nu=1.5), GP_RBF(ARD=True)):
        with pytest.raises(RuntimeError, match="fit"):
            g.leave_one_out()
        with pytest.raises(RuntimeError, match="fit"):
            g.loo_log_predictive_density()
