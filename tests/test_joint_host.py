"""CPU tests of the joint predictive distribution (include/cimrgp_joint.h): the generator phi restated in NumPy against
Philox4x32-10 known answers and its promised invariances, the header's symbols, argument validation without a GPU and
the index-set checks of the model's joint methods.  phi is imported by the GPU tests."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of uint32 values, key: 2; returns the 4 output words as uint64 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for r in range(10):
        if r:
            k0 = (k0 + W0) & MASK
            k1 = (k1 + W1) & MASK
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def phi(seed, key, cols, ns, col0=0):
    """(cols x ns) array: phi(seed, key, col0 + c, i)."""
    c = np.arange(col0, col0 + cols, dtype=np.uint64)[:, None]
    i = np.arange(ns, dtype=np.uint64)[None, :]
    key = int(key)
    seed = int(seed)
    shape = (cols, ns)
    x = philox4x32_10([np.broadcast_to(i >> np.uint64(1), shape), np.broadcast_to(c, shape), key & 0xFFFFFFFF, key >> 32],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    u1 = (((x[1] << np.uint64(32)) | x[0]) >> np.uint64(11)).astype(np.float64)
    u2 = (((x[3] << np.uint64(32)) | x[2]) >> np.uint64(11)).astype(np.float64)
    u1 = (u1 + 0.5) * 2.0 ** -53
    u2 = (u2 + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return np.where((np.broadcast_to(i, shape) & np.uint64(1)) == 0, r * np.cos(a), r * np.sin(a))


# ---- Philox4x32-10 known answers (the round function alone) ----
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(ctr, key)
    assert tuple(int(v) for v in got) == want


def test_phi_invariances():
    seed, key = 12345, (3 << 32) + 7
    full = phi(seed, key, 20, 101)
    # a column prefix, a point prefix and a column window are the same values
    np.testing.assert_array_equal(phi(seed, key, 5, 101), full[:5])
    np.testing.assert_array_equal(phi(seed, key, 20, 37), full[:, :37])
    np.testing.assert_array_equal(phi(seed, key, 6, 101, col0=9), full[9:15])
    # independent of the other blocks (batch order): a block's values depend on its key alone
    other = phi(seed, key + 1, 20, 101)
    assert not np.any(other == full)
    assert not np.any(phi(seed + 1, key, 20, 101) == full)
    # pairs (2m, 2m + 1) share one Philox output: cos and sin of one angle
    r2 = full[:, 0:100:2] ** 2 + full[:, 1:101:2] ** 2
    x = philox4x32_10([0, 0, key & 0xFFFFFFFF, key >> 32], [seed, 0])
    u1 = ((((int(x[1]) << 32) | int(x[0])) >> 11) + 0.5) * 2.0 ** -53
    assert r2[0, 0] == pytest.approx(-2.0 * np.log(u1), rel=1e-14)
    z = phi(7, 0, 200, 500).ravel()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02


def _joint_header_symbols():
    text = open(os.path.join(ROOT, "include", "cimrgp_joint.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cimrgp_[a-z0-9_]+)\s*\(", text)))


def test_joint_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    names = _joint_header_symbols()
    assert names == ["cimrgp_layer_joint_cov", "cimrgp_layer_sample", "cimrgp_normal_fill"]
    assert sorted(_lib.JOINT_SIGNATURES) == names
    for name in names:
        assert hasattr(lib, name), name
    main = open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert '#include "cimrgp_joint.h"' in main


def _buf():
    buf = (ctypes.c_double * 4096)()
    return buf, ctypes.addressof(buf)


def test_normal_fill_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    rc = lib.cimrgp_normal_fill(7, 0, p, 1, 0, 4, 8, p, 8, 32, None)
    assert rc < 0 and "cimrgp_normal_fill" in _lib.last_error() and "dtype" in _lib.last_error()
    rc = lib.cimrgp_normal_fill(_lib.F64, 0, p, 1, 0, -1, 8, p, 8, 32, None)
    assert rc < 0 and "negative size" in _lib.last_error()
    rc = lib.cimrgp_normal_fill(_lib.F64, 0, p, 1, 0, 4, 8, p, 6, 32, None)
    assert rc < 0 and "leading dimension" in _lib.last_error()
    rc = lib.cimrgp_normal_fill(_lib.F64, 0, p, 2, 0, 4, 8, p, 8, 16, None)
    assert rc < 0 and "stride" in _lib.last_error()


def test_joint_cov_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    args = dict(dtype=_lib.F64, cov=_lib.COV_RBF, n=16, d=1, ns=8, batch=1, ldl=16, ldw=16, ldc=8)

    def call(**kw):
        a = dict(args, **kw)
        return lib.cimrgp_layer_joint_cov(a["dtype"], a["cov"], p, p, a["n"], a["d"], p, p, a["ns"], a["batch"], 1.0, 1.0, p,
                                          a["ldl"], 256, p, 1 << 20, None, p, a["ldw"], 256, p, a["ldc"], 64, None, 0, None, None)
    assert call(dtype=9) < 0 and "cimrgp_layer_joint_cov" in _lib.last_error() and "dtype" in _lib.last_error()
    assert call(cov=11) < 0 and "unknown covariance" in _lib.last_error()
    assert call(d=9) < 0 and "input dimension" in _lib.last_error()
    assert call(ldc=4) < 0 and "leading dimension" in _lib.last_error()
    assert call(ldw=17) < 0 and "16 bytes" in _lib.last_error()
    # a factor workspace without info
    rc = lib.cimrgp_layer_joint_cov(_lib.F64, 0, p, p, 16, 1, p, p, 8, 1, 1.0, 1.0, p, 16, 256, p, 1 << 20, None, p, 16, 256,
                                    p, 8, 64, p, 1 << 20, None, None)
    assert rc < 0 and "info" in _lib.last_error()


def test_layer_sample_argument_errors():
    lib = _lib.load()
    buf, p = _buf()
    assert lib.cimrgp_layer_sample(5, p, 8, 64, 8, 1, p, 8, 64, 4, p, p, 8, None) < 0
    assert "cimrgp_layer_sample" in _lib.last_error() and "dtype" in _lib.last_error()
    assert lib.cimrgp_layer_sample(_lib.F64, p, 8, 64, 8, 1, p, 8, 64, -1, p, p, 8, None) < 0
    assert "dimensions" in _lib.last_error()
    assert lib.cimrgp_layer_sample(_lib.F64, p, 8, 64, 8, 1, p, 6, 64, 4, p, p, 8, None) < 0
    assert "leading dimension" in _lib.last_error()
    assert lib.cimrgp_layer_sample(_lib.F64, None, 8, 64, 8, 1, p, 8, 64, 4, p, p, 8, None) < 0
    assert "null pointer" in _lib.last_error()


def test_joint_methods_check_the_index_set_like_get_predicted_mean():
    import cimrgp_amd as ca
    from cimrgp_amd.MRGP import MultiResolutionGaussianProcess
    m = object.__new__(MultiResolutionGaussianProcess)
    m.index_set_obj = ca.IndexSetUniform(256, 2, 2)
    m.n_regions = [len(b) for b in m.index_set_obj.bounds]
    xs = np.zeros((64, 1))
    for bad, nr in ((ca.IndexSetUniform(64, 3, 2), None), (ca.IndexSetUniform(64, 2, 4), None),
                    (ca.IndexSetUniform(64, 2, 2), [1, 2, 3])):
        with pytest.raises(ValueError) as ref:
            m.get_predicted_mean(xs, bad, nr)
        with pytest.raises(ValueError) as e1:
            m.get_predicted_covariance(xs, bad, nr)
        with pytest.raises(ValueError) as e2:
            m.posterior_samples(xs, 3, bad, nr)
        assert str(e1.value) == str(ref.value) == str(e2.value)
