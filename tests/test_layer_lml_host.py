"""The batched layer objective (cimrgp_layer_lml_grad_cov) and the model's hyper-parameter option: symbols and
argument checks that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cimrgp_layer_lml_grad_cov", "cimrgp_layer_lml_grad_scratch_bytes")


def _symbols(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cimrgp_[a-z0-9_]+)\s*\(", text)))


def test_new_symbols_in_their_header_library_and_signatures():
    """include/cimrgp_objective.h (included by cimrgp.h) declares exactly the layer objective's entry points; the library
    exports them and _lib.OBJECTIVE_SIGNATURES lists them, apart from the fit / prediction ABI of cimrgp.h."""
    lib = _lib.load()
    assert _symbols("cimrgp_objective.h") == sorted(NEW) == sorted(_lib.OBJECTIVE_SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in _symbols("cimrgp.h") and name not in _lib.SIGNATURES
    assert '#include "cimrgp_objective.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()


def _call(lib, cov=_lib.COV_RBF, batch=2, null_x=False, n=64):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    info = (ctypes.c_int32 * 4)()
    return lib.cimrgp_layer_lml_grad_cov(_lib.F64, cov, None if null_x else p, p, None, p, batch, n, 1, 2, 1.0, 1.0, 0.1, None,
                                         p, 64, 64 * 64, p, p, 1 << 30, ctypes.addressof(info), p, p, None)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _call(lib, cov=17) < 0
    msg = _lib.last_error()
    assert "cimrgp_layer_lml_grad_cov" in msg and "covariance" in msg
    assert _call(lib, batch=0) < 0
    assert "cimrgp_layer_lml_grad_cov" in _lib.last_error() and "dimensions" in _lib.last_error()
    assert _call(lib, null_x=True) < 0
    assert "cimrgp_layer_lml_grad_cov" in _lib.last_error() and "null pointer" in _lib.last_error()


def test_scratch_bytes():
    lib = _lib.load()
    assert lib.cimrgp_layer_lml_grad_scratch_bytes(_lib.F64, 0, 2, 1) == 0
    assert lib.cimrgp_layer_lml_grad_scratch_bytes(7, 64, 2, 1) == 0
    one = lib.cimrgp_layer_lml_grad_scratch_bytes(_lib.F64, 300, 2, 1)
    # carried rows (q + n) x ld, z, alpha, solve work, bias, noise, tile records
    assert one >= (302 * 304 + 4 * 300 * 2 + 3) * 8
    assert lib.cimrgp_layer_lml_grad_scratch_bytes(_lib.F64, 300, 2, 8) >= 8 * one - 8 * 256 * 7
    assert lib.cimrgp_layer_lml_grad_scratch_bytes(_lib.F32, 300, 2, 1) < one


def test_device_wrapper_refuses_unknown_covariance_before_allocating():
    from cimrgp_amd import device as dev
    with pytest.raises(ValueError, match="covariance"):
        dev.layer_lml_grad(None, None, None, None, 64, 1.0, 1.0, 0.1, None, None, None, None, None, None, cov=9)


def _tiny():
    import cimrgp_amd as ca
    rng = np.random.default_rng(0)
    n = 64
    x = rng.uniform(size=(n, 1))
    y = rng.normal(size=(n, 2))
    return ca, [x, y], ca.IndexSetUniform(n, 1, 2)


def test_model_rejects_optimisation_with_a_basis_object():
    ca, xy, idx = _tiny()
    with pytest.raises(TypeError, match="not yet supported"):
        ca.MultiResolutionGaussianProcess(xy, n_basis=4, index_set_obj=idx, basis_function_obj=ca.LaplacianEigenpairs(),
                                          spectral_density_obj=ca.MaternKernel(nu=1, l=1, sf=1),
                                          optimize_hyperparameters=True)


def test_model_rejects_zero_iterations():
    ca, xy, idx = _tiny()
    with pytest.raises(ValueError, match="max_iters"):
        ca.MultiResolutionGaussianProcess(xy, index_set_obj=idx, optimize_hyperparameters=True, max_iters=0)
