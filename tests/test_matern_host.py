"""DenseMaternKernel (half-integer Matern of the dense path) and the covariance entry points of the C ABI,
without a GPU: the reference's Matern values, the link to the reduced-rank model, argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import cimrgp_amd as ca
from cimrgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cimrgp_cov_gram", "cimrgp_cov_cross", "cimrgp_cov_predict_mean", "cimrgp_cov_lml_grad",
               "cimrgp_cov_lml_grad_ard", "cimrgp_layer_fit_cov", "cimrgp_layer_predict_cov"]


def test_dense_matern_matches_reference_matern(golden_dir):
    g = np.load(os.path.join(golden_dir, "kernel_objects.npz"))
    for nu in (0.5, 1.5, 2.5):
        k = ca.DenseMaternKernel(nu=nu, l=0.7, sf=1.3)
        tag = str(nu).replace(".", "p")
        np.testing.assert_allclose(k.kernel(g["mat_r"]), g["mat_k_" + tag], rtol=1e-12)
        np.testing.assert_allclose(k.log_kernel(g["mat_r"]), g["mat_lk_" + tag], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(k.spectral(g["mat_s"]), g["mat_s_" + tag], rtol=1e-12)
        np.testing.assert_allclose(k.log_spectral(g["mat_s"]), g["mat_ls_" + tag], rtol=1e-12, atol=1e-13)
    k = ca.DenseMaternKernel(nu=1.5, l=0.7, sf=1.3)
    np.testing.assert_allclose(k.estimate_kernel(g["est_phi_a"], g["est_phi_b"], g["est_lambda"]), g["est_out"], rtol=1e-12)


def test_dense_matern_protocol_and_edge_cases():
    for nu, cov in ((0.5, _lib.COV_MATERN12), (1.5, _lib.COV_MATERN32), (2.5, _lib.COV_MATERN52)):
        k = ca.DenseMaternKernel(nu=nu, l=0.4, sf=2.5, noise=0.1)
        assert (k.nu, k.l, k.sf, k.noise, k.name, k.cov) == (nu, 0.4, 2.5, 0.1, "Matern", cov)
        assert k.kernel(0.0) == 2.5
        assert k.kernel(np.zeros(3)).tolist() == [2.5] * 3
        assert np.all(np.diff(k.kernel(np.linspace(0, 3, 50))) < 0)
        k2 = k.with_noise(0.3)
        assert isinstance(k2, ca.DenseMaternKernel) and (k2.nu, k2.l, k2.sf, k2.noise) == (nu, 0.4, 2.5, 0.3)
    r = np.linspace(0, 2, 9)
    np.testing.assert_allclose(ca.DenseMaternKernel(0.5, 0.5, 1.0).kernel(r), np.exp(-2 * r), rtol=1e-15)
    t = np.sqrt(3) * r / 0.5
    np.testing.assert_allclose(ca.DenseMaternKernel(1.5, 0.5, 2.0).kernel(r), 2 * (1 + t) * np.exp(-t), rtol=1e-14)
    assert ca.RBFKernel().cov == _lib.COV_RBF
    k3 = ca.RBFKernel(0.3, 1.7).with_noise(0.2)
    assert isinstance(k3, ca.RBFKernel) and (k3.l, k3.sf, k3.noise) == (0.3, 1.7, 0.2)
    for bad in (dict(nu=1.0), dict(nu=3.5), dict(l=0.0), dict(l=-1.0), dict(sf=0.0), dict(sf=-2.0)):
        with pytest.raises(ValueError):
            ca.DenseMaternKernel(**bad)
    with pytest.raises(ValueError):
        ca.GP_Matern(nu=2.0)


@pytest.mark.parametrize("nu,m,bar", [(1.5, 400, 2e-5), (2.5, 400, 2e-6), (0.5, 1600, 3e-3)])
def test_reduced_rank_estimate_converges_to_dense_matern(nu, m, bar):
    """The reduced-rank model's kernel (sum over the Laplacian basis on [-L, L], weights from the spectral
    density) is the dense Matern up to the reference's sqrt(2) (see test_rbf_kernel_protocol)."""
    k = ca.DenseMaternKernel(nu=nu, l=0.7, sf=1.3)
    x = np.linspace(-1.0, 1.0, 41)[:, None]
    lap = ca.LaplacianEigenpairs()
    pairs = [lap.get_eigenpairs(x, j, basis_interval=np.array([4.0])) for j in range(1, m + 1)]
    phi = np.stack([f for f, _ in pairs], axis=1)
    lam = np.array([lm for _, lm in pairs])
    est = np.sqrt(2) * np.stack([k.estimate_kernel(phi, np.repeat(phi[i:i + 1], 41, axis=0), lam) for i in range(41)])
    err = np.max(np.abs(est - k.kernel(np.abs(x - x.T)))) / k.sf
    assert err < bar, err


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(cimrgp_[a-z0-9_]+)\s*\(", text))


def test_cov_symbols_in_header_library_and_signatures():
    lib = _lib.load()
    names = _header_symbols()
    assert len(names) == 54
    for name in NEW_SYMBOLS:
        assert name in names and name in _lib.SIGNATURES and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    for name, v in (("RBF", 0), ("MATERN12", 1), ("MATERN32", 2), ("MATERN52", 3)):
        m = re.search(r"#define\s+CIMRGP_COV_%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == v == getattr(_lib, "COV_" + name)


def test_cov_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    F64, M32 = _lib.F64, _lib.COV_MATERN32

    def err(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, _lib.last_error())

    # null pointers
    err(lib.cimrgp_cov_gram(F64, M32, None, 4, 1, 1.0, 1.0, 0.0, p, 4, 0, None), "null pointer")
    err(lib.cimrgp_cov_cross(F64, M32, p, 4, None, 4, 1, 1.0, 1.0, p, 4, None), "null pointer")
    err(lib.cimrgp_cov_predict_mean(F64, M32, p, 4, 1, None, 1, p, 4, 1.0, 1.0, None, p, 0, None), "null pointer")
    err(lib.cimrgp_cov_lml_grad(F64, M32, p, 4, 1, None, 4, p, 1, 1.0, 1.0, 0.1, p, p, None), "null pointer")
    err(lib.cimrgp_cov_lml_grad_ard(F64, M32, p, 4, 1, p, 4, p, 1, 1.0, 0.1, None, p, None), "null pointer")
    err(lib.cimrgp_layer_fit_cov(F64, M32, None, p, None, p, p, 1, 4, 1, 1, 1.0, 1.0, -1.0, 0.01, 1e-8, None, None,
                                 p, 4, 16, p, 1 << 20, p, p, 4, p, p, p, p, p, None), "null pointer")
    err(lib.cimrgp_layer_predict_cov(F64, M32, p, None, 4, 1, p, p, 4, 1, 1.0, 1.0, p, 4, 16, p, 1 << 20, p, 1, None, None,
                                     p, 4, 16, p, p, None), "null pointer")
    # unknown covariance: rejected before any device work
    for cov in (-1, 4, 99):
        err(lib.cimrgp_cov_gram(F64, cov, p, 4, 1, 1.0, 1.0, 0.0, p, 4, 0, None), "covariance")
        err(lib.cimrgp_cov_cross(F64, cov, p, 4, p, 4, 1, 1.0, 1.0, p, 4, None), "covariance")
        err(lib.cimrgp_cov_predict_mean(F64, cov, p, 4, 1, p, 1, p, 4, 1.0, 1.0, None, p, 0, None), "covariance")
        err(lib.cimrgp_cov_lml_grad(F64, cov, p, 4, 1, p, 4, p, 1, 1.0, 1.0, 0.1, p, p, None), "covariance")
        err(lib.cimrgp_cov_lml_grad_ard(F64, cov, p, 4, 1, p, 4, p, 1, 1.0, 0.1, p, p, None), "covariance")
        err(lib.cimrgp_layer_fit_cov(F64, cov, p, p, None, p, p, 1, 4, 1, 1, 1.0, 1.0, -1.0, 0.01, 1e-8, None, None,
                                     p, 4, 16, p, 1 << 20, p, p, 4, p, p, p, p, p, None), "covariance")
        err(lib.cimrgp_layer_predict_cov(F64, cov, p, p, 4, 1, p, p, 4, 1, 1.0, 1.0, p, 4, 16, p, 1 << 20, p, 1, None,
                                         None, p, 4, 16, p, p, None), "covariance")
    # non-positive length-scales and bad dimensions
    for cov in (_lib.COV_MATERN12, M32, _lib.COV_MATERN52):
        err(lib.cimrgp_cov_gram(F64, cov, p, 4, 1, 0.0, 1.0, 0.0, p, 4, 0, None), "length-scale")
        err(lib.cimrgp_cov_cross(F64, cov, p, 4, p, 4, 1, -1.0, 1.0, p, 4, None), "length-scale")
        err(lib.cimrgp_cov_predict_mean(F64, cov, p, 4, 1, p, 1, p, 4, 0.0, 1.0, None, p, 0, None), "length-scale")
        err(lib.cimrgp_cov_lml_grad(F64, cov, p, 4, 1, p, 4, p, 1, -0.5, 1.0, 0.1, p, p, None), "length-scale")
        err(lib.cimrgp_cov_gram(F64, cov, p, 4, 9, 1.0, 1.0, 0.0, p, 4, 0, None), "dimension")
    err(lib.cimrgp_cov_gram(7, M32, p, 4, 1, 1.0, 1.0, 0.0, p, 4, 0, None), "dtype")
    with pytest.raises(_lib.CimrgpError, match="covariance"):
        _lib.check(lib.cimrgp_cov_gram(F64, 5, p, 4, 1, 1.0, 1.0, 0.0, p, 4, 0, None), "cimrgp_cov_gram")


def test_model_accepts_dense_matern_kernels():
    """The type check lets DenseMaternKernel through (alone or in a mixed per-layer list); MaternKernel (general nu,
    no closed form) is still refused.  Without a device the model then stops at the no-GPU RuntimeError."""
    import torch
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(0, 1, size=(64, 1)), axis=0)
    y = np.hstack([np.sin(3 * x), np.cos(3 * x)])
    idx = ca.IndexSetUniform(64, 2, 2)
    with pytest.raises(TypeError):
        ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=ca.MaternKernel(nu=1.5))
    for spec in (ca.DenseMaternKernel(), [ca.DenseMaternKernel(0.5), ca.RBFKernel(), ca.DenseMaternKernel(2.5)]):
        if torch.cuda.is_available():
            continue
        with pytest.raises(RuntimeError, match="no HIP device"):
            ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=spec)


def test_cov_errors_name_the_entry_point_called():
    """An error of a covariance entry point names that entry point, whatever the covariance (the RBF included)."""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    F64 = _lib.F64
    for cov in (_lib.COV_RBF, _lib.COV_MATERN52):
        assert lib.cimrgp_cov_gram(F64, cov, p, 4, 1, 0.0, 1.0, 0.0, p, 4, 0, None) < 0
        assert _lib.last_error().startswith("cimrgp_cov_gram:"), _lib.last_error()
        assert lib.cimrgp_cov_cross(F64, cov, p, 4, p, 4, 9, 1.0, 1.0, p, 4, None) < 0
        assert _lib.last_error().startswith("cimrgp_cov_cross:"), _lib.last_error()
        assert lib.cimrgp_cov_predict_mean(F64, cov, p, 4, 1, p, 9, p, 4, 1.0, 1.0, None, p, 0, None) < 0
        assert _lib.last_error().startswith("cimrgp_cov_predict_mean:"), _lib.last_error()
        assert lib.cimrgp_cov_lml_grad(F64, cov, p, 4, 9, p, 4, p, 1, 1.0, 1.0, 0.1, p, p, None) < 0
        assert _lib.last_error().startswith("cimrgp_cov_lml_grad:"), _lib.last_error()
        assert lib.cimrgp_cov_lml_grad_ard(F64, cov, p, 4, 9, p, 4, p, 1, 1.0, 0.1, p, p, None) < 0
        assert _lib.last_error().startswith("cimrgp_cov_lml_grad_ard:"), _lib.last_error()
    # the RBF entry points keep their own names
    assert lib.cimrgp_rbf_gram(F64, p, 4, 1, 0.0, 1.0, 0.0, p, 4, 0, None) < 0
    assert _lib.last_error().startswith("cimrgp_rbf_gram:")
    assert lib.cimrgp_lml_grad_ard(F64, p, 4, 9, p, 4, p, 1, 1.0, 0.1, p, p, None) < 0
    assert _lib.last_error().startswith("cimrgp_lml_grad:")


def test_device_wrappers_refuse_unknown_covariance_before_any_allocation():
    import torch
    from cimrgp_amd import device as dev
    x = torch.zeros((4, 1), dtype=torch.float64)          # a host tensor: any device work would fail differently
    for call in (lambda: dev.rbf_gram(x, 1.0, 1.0, cov=4), lambda: dev.rbf_cross(x, x, 1.0, 1.0, cov=-1),
                 lambda: dev.predict_mean(x, x, x, 1.0, 1.0, cov=9),
                 lambda: dev.lml_grad(x, x, 4, x, 1.0, 1.0, 0.1, cov=5),
                 lambda: dev.lml_grad_ard(x, x, 4, x, 1.0, 0.1, cov=5),
                 lambda: dev.layer_fit(x, x, None, x, x, 4, 1.0, 1.0, -1.0, 0.01, 1e-8, None, None, x, x, x, x, x, x, x,
                                       cov=6),
                 lambda: dev.layer_predict(x, x, 4, x, x, 4, 1.0, 1.0, x, x, x, x, None, x, x, cov=6)):
        with pytest.raises(ValueError, match="unknown covariance"):
            call()
