"""ARD length-scales for the model's layers, the part that needs no GPU: the kernel objects with a length-scale vector, the
header include/cimrgp_layer_ard.h with its signature table, every refusal of cimrgp_layer_lml_grad_ard_cov that comes before
any HIP call (a literal table in the manner of tests/test_sparse_layer_refusals_host.py), the model constructor's check,
and the host rules of Hyper.py at d + 2 parameters -- the widened [lml | grad | failure] all-reduce buffer included, which
the two-rank GPU test of tests/test_gpu_model_ard.py also crosses."""
import os
import re

import numpy as np
import pytest

import cimrgp_amd as ca
from cimrgp_amd import Hyper, KernelClass, _lib
from test_sparse_refusals_host import _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = 'cimrgp_layer_lml_grad_ard_cov'


# ---- kernel objects ---------------------------------------------------------------------------------------------------------
def _makers():
    return [lambda **kw: ca.RBFKernel(**kw)] + [lambda nu=nu, **kw: ca.DenseMaternKernel(nu, **kw) for nu in (0.5, 1.5, 2.5)]


@pytest.mark.parametrize("make", _makers())
def test_scalar_length_scale_is_a_float_and_not_ard(make):
    for l in (0.5, 2, np.float64(0.5), np.array(0.5)):
        k = make(l=l, sf=1.5)
        assert type(k.l) is float and k.l == float(l) and k.ard is False
        assert k.l == 0.5 or k.l == 2.0
        assert np.isfinite(k.kernel(0.3)) and np.isfinite(k.log_spectral(0.3))
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='^length-scale must be positive$'):
            make(l=bad)


@pytest.mark.parametrize("make", _makers())
def test_vector_length_scale_makes_an_ard_kernel(make):
    given = [0.5, 2.0]
    k = make(l=given, sf=1.5, noise=0.1)
    assert isinstance(k.l, np.ndarray) and k.l.dtype == np.float64 and k.l.shape == (2,) and k.ard is True
    assert np.array_equal(k.l, [0.5, 2.0])
    arr = np.array([0.5, 2.0, 1.0])
    k3 = make(l=arr)
    arr[0] = 9.0
    assert np.array_equal(k3.l, [0.5, 2.0, 1.0])                      # a fresh array: the caller's is not aliased
    assert make(l=(0.7,)).ard is True and make(l=(0.7,)).l.shape == (1,)
    assert make(l=np.linspace(0.5, 1.2, KernelClass.MAXD)).l.shape == (KernelClass.MAXD,)
    for bad in ([0.5, 0.0], [0.5, -1.0], [np.nan, 1.0], [np.inf, 1.0]):
        with pytest.raises(ValueError, match='^length-scale must be positive$'):
            make(l=bad)
    with pytest.raises(ValueError):
        make(l=np.ones(KernelClass.MAXD + 1))
    with pytest.raises(ValueError):
        make(l=[])
    with pytest.raises(ValueError):
        make(l=np.ones((2, 2)))
    assert KernelClass.MAXD == 8


@pytest.mark.parametrize("make", _makers())
def test_with_values_and_with_noise_keep_what_they_are_given(make):
    k = make(l=[0.5, 2.0], sf=1.5)
    n = k.with_noise(0.2)
    assert type(n) is type(k) and n.ard and np.array_equal(n.l, k.l) and n.l is not k.l and (n.sf, n.noise, n.cov) == (1.5, 0.2, k.cov)
    v = k.with_values(np.array([0.3, 0.4]), 2.0, 0.01)
    assert type(v) is type(k) and v.ard and np.array_equal(v.l, [0.3, 0.4]) and (v.sf, v.noise) == (2.0, 0.01)
    s = k.with_values(0.7, 2.0, None)                                 # a scalar gives an isotropic kernel
    assert type(s.l) is float and s.l == 0.7 and s.ard is False and s.noise is None
    back = s.with_values([1.0, 1.0], 1.0, None)
    assert back.ard and np.array_equal(back.l, [1.0, 1.0])
    assert getattr(v, 'nu', None) == getattr(k, 'nu', None)
    assert np.array_equal(k.l, [0.5, 2.0]) and k.noise is None        # the old object is as it was


@pytest.mark.parametrize("make", _makers())
def test_scalar_distance_protocol_is_refused_on_an_ard_kernel(make):
    k = make(l=[0.5, 2.0])
    phi = np.ones((3, 2))
    for call in (lambda: k.kernel(0.3), lambda: k.log_kernel(0.3), lambda: k.spectral(0.3), lambda: k.log_spectral(0.3),
                 lambda: k.estimate_kernel(phi, phi, np.ones(2))):
        with pytest.raises(TypeError, match='^not yet supported$'):
            call()


def test_sparse_kernel_forwards_ard():
    s = ca.SparseKernel(ca.RBFKernel(l=[0.5, 2.0], sf=1.5), num_inducing=7, approximation='vfe')
    assert s.ard is True and np.array_equal(s.l, [0.5, 2.0]) and (s.sf, s.noise, s.cov) == (1.5, None, 0)
    t = s.with_values([0.1, 0.2], 1.0, 0.3)
    assert t.ard and np.array_equal(t.l, [0.1, 0.2]) and (t.num_inducing, t.approximation) == (7, 'vfe')
    assert s.with_noise(0.2).ard and np.array_equal(s.with_noise(0.2).l, [0.5, 2.0])
    assert s.with_values(0.4, 1.0, None).ard is False
    assert ca.SparseKernel(ca.DenseMaternKernel(1.5, l=0.3)).ard is False


def test_dense_block_refuses_an_ard_kernel():
    import torch
    from cimrgp_amd.Posteriors import DenseBlock
    x = torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(TypeError, match='isotropic kernel'):
        DenseBlock(x, ca.RBFKernel(l=[0.5, 2.0]))
    assert DenseBlock(x, ca.RBFKernel(l=[0.5, 2.0]).with_values(1.0, 1.0, None)).n == 4


def test_gram_of_an_ard_kernel_refuses_inputs_of_another_dimension():
    import torch
    k = ca.RBFKernel(l=[0.5, 2.0])
    with pytest.raises(ValueError):
        k.gram(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        ca.DenseMaternKernel(1.5, l=[0.5, 2.0]).gram(torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 1), dtype=torch.float64))


# ---- the header and its table -----------------------------------------------------------------------------------------------
BASE = [('dtype', 1), ('cov', 0), ('xs', 'P'), ('y', 'P'), ('fbar', 'P'), ('starts', 'P'), ('batch', 3), ('n', 200), ('d', 2),
        ('q', 2), ('sf2', 1.0), ('noise', 0.1), ('shared_bias', None), ('k_arena', 'P'), ('ldk', 208), ('k_stride', 200 * 208),
        ('kinv_arena', 'P'), ('ws_arena', 'P'), ('ws_stride', 1 << 20), ('info', 'P'), ('scratch', 'P'), ('out', 'P'),
        ('stream', None)]

ROWS = [
    ({'dtype': 7}, -1, FN + ': unknown dtype'),
    ({'cov': 4}, -1, FN + ': unknown covariance'),
    ({'cov': -1}, -1, FN + ': unknown covariance'),
    ({'xs': None}, -1, FN + ': null pointer'),
    ({'y': None}, -1, FN + ': null pointer'),
    ({'starts': None}, -1, FN + ': null pointer'),
    ({'k_arena': None}, -1, FN + ': null pointer'),
    ({'kinv_arena': None}, -1, FN + ': null pointer'),
    ({'ws_arena': None}, -1, FN + ': null pointer'),
    ({'info': None}, -1, FN + ': null pointer'),
    ({'scratch': None}, -1, FN + ': null pointer'),
    ({'out': None}, -1, FN + ': null pointer'),
    ({'n': 0}, -1, FN + ': bad dimensions'),
    ({'n': 1 << 30}, -1, FN + ': bad dimensions'),
    ({'d': 0}, -1, FN + ': input dimension must be in [1, 8]'),
    ({'d': 9}, -1, FN + ': input dimension must be in [1, 8]'),
    ({'q': 0}, -1, FN + ': number of outputs must be in [1, 8]'),
    ({'q': 9}, -1, FN + ': number of outputs must be in [1, 8]'),
    ({'batch': 0}, -1, FN + ': bad dimensions'),
    ({'batch': 65536}, -1, FN + ': bad dimensions'),
    ({'ldk': 199}, -1, FN + ': bad dimensions'),
    ({'ldk': 201}, -1, FN + ': leading dimensions and strides must be multiples of 16 bytes'),
    ({'k_stride': 200 * 208 + 1}, -1, FN + ': leading dimensions and strides must be multiples of 16 bytes'),
    ({'k_stride': 100 * 208}, -1, FN + ': matrix stride too small'),
    ({'k_arena': 'P+8'}, -1, FN + ': pointers must be 16-byte aligned'),
    ({'scratch': 'P+8'}, -1, FN + ': pointers must be 16-byte aligned'),
    ({'ws_stride': 16}, -1, FN + ': workspace stride too small or misaligned'),
    ({'ws_stride': (1 << 20) + 8}, -1, FN + ': workspace stride too small or misaligned'),
    ({'sf2': 0.0}, -1, FN + ': kernel parameters must be positive (noise non-negative)'),
    ({'noise': -1e-3}, -1, FN + ': kernel parameters must be positive (noise non-negative)'),
    # several faults at once: the first check in the order of the call decides
    ({'dtype': 7, 'cov': 9, 'xs': None, 'n': 0, 'd': 0, 'q': 0}, -1, FN + ': null pointer'),
    ({'dtype': 7, 'cov': 9, 'n': 0, 'd': 0}, -1, FN + ': unknown covariance'),
    ({'dtype': 7, 'n': 0, 'd': 0, 'q': 0}, -1, FN + ': unknown dtype'),
    ({'n': 0, 'd': 9, 'q': 9, 'sf2': -1.0}, -1, FN + ': bad dimensions'),
    ({'d': 9, 'q': 9, 'ldk': 201}, -1, FN + ': input dimension must be in [1, 8]'),
    ({'q': 9, 'k_stride': 8, 'sf2': -1.0}, -1, FN + ': number of outputs must be in [1, 8]'),
]


def test_layer_ard_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_layer_ard.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_layer_lml_grad_ard_cov", "cimrgp_layer_lml_grad_ard_scratch_bytes"] == sorted(_lib.LAYER_ARD_SIGNATURES)
    for name in names:
        assert getattr(lib, name).argtypes == _lib.LAYER_ARD_SIGNATURES[name][1], name
    assert '#include "cimrgp_layer_ard.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert len(BASE) == len(_lib.LAYER_ARD_SIGNATURES[FN][1])
    # the twin without its `ell`
    assert len(_lib.LAYER_ARD_SIGNATURES[FN][1]) == len(_lib.OBJECTIVE_SIGNATURES["cimrgp_layer_lml_grad_cov"][1]) - 1
    assert _lib.LAYER_ARD_SIGNATURES[FN[:-3] + "scratch_bytes"] == _lib.OBJECTIVE_SIGNATURES["cimrgp_layer_lml_grad_scratch_bytes"]


def test_layer_ard_refusals_status_and_text():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE]
    for broken, status, text in ROWS:
        assert broken and set(broken) <= set(keys), broken
        args = [broken.get(k, v) for k, v in BASE]
        args = [stand_in.get(a, a) if isinstance(a, str) else a for a in args]
        rc = getattr(lib, FN)(*args)
        print(broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), broken


def test_layer_ard_scratch_bytes():
    lib = _lib.load()
    ard, iso = lib.cimrgp_layer_lml_grad_ard_scratch_bytes, lib.cimrgp_layer_lml_grad_scratch_bytes
    for bad in ((7, 200, 2, 3), (1, 0, 2, 3), (1, -5, 2, 3), (1, 200, 0, 3), (1, 200, 2, 0)):
        assert ard(*bad) == 0, bad
    for dtype in (0, 1):
        for n, q, batch in ((1, 1, 1), (65, 2, 1), (200, 2, 3), (1025, 8, 5)):
            a, i = ard(dtype, n, q, batch), iso(dtype, n, q, batch)
            tiles = ((n + 63) // 64) * ((n + 63) // 64 + 1) // 2
            assert a >= i > 0 and a % 256 == 0
            # the tile records alone differ: 10 doubles per tile instead of 3, each segment rounded up to 256 bytes
            up = lambda b: (b + 255) // 256 * 256
            assert a - i == up(batch * tiles * 10 * 8) - up(batch * tiles * 3 * 8), (dtype, n, q, batch)


# ---- the model's constructor -----------------------------------------------------------------------------------------------
def _xy(d, n=64):
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, size=(n, d))
    return x, np.hstack([np.sin(3 * x[:, :1]), np.cos(3 * x[:, -1:])])


def test_model_refuses_an_ard_kernel_of_another_dimension_without_a_gpu():
    x, y = _xy(2)
    idx = ca.IndexSetUniform(64, 2, 2)
    for spec in (ca.RBFKernel(l=[0.5, 1.0, 2.0]), [ca.RBFKernel(), ca.DenseMaternKernel(1.5, l=[0.5]), ca.RBFKernel(l=[1.0, 1.0])],
                 [ca.RBFKernel(), ca.RBFKernel(), ca.SparseKernel(ca.RBFKernel(l=[0.5, 1.0, 2.0]), num_inducing=8)]):
        with pytest.raises(ValueError, match='length-scales'):
            ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=spec)


def test_model_takes_ard_kernels_up_to_the_device_check():
    """Without a device the constructor gets past every host check and stops at the no-GPU RuntimeError; with one it goes
    on and builds the layer objects around the ARD kernels (the fits are in tests/test_gpu_model_ard.py)."""
    import torch
    x, y = _xy(2)
    idx = ca.IndexSetUniform(64, 2, 2)
    specs = (ca.RBFKernel(l=[0.5, 2.0]), [ca.DenseMaternKernel(0.5, l=[0.5, 2.0]), ca.RBFKernel(), ca.RBFKernel(l=[1.0, 1.0])],
             [ca.SparseKernel(ca.RBFKernel(l=[0.5, 2.0]), num_inducing=8), ca.RBFKernel(l=[1.0, 1.0]), ca.RBFKernel()])
    cases = [(spec, kw) for spec in specs for kw in ({}, dict(snr_ratio=10.0), dict(optimize_hyperparameters=True))]
    cases.append((specs[0], dict(dtype='f32')))
    for spec, kw in cases:
        build = lambda: ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=spec, **kw)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no HIP device"):
                build()
            continue
        model = build()
        want = [k.ard for k in (spec if isinstance(spec, list) else [spec] * 3)]
        assert [p.kernel.ard for p in model.posterior_obj] == want
        k0 = model.posterior_obj[0].kernel
        assert np.array_equal(k0.l, [0.5, 2.0]) and (k0.noise is not None) == ('snr_ratio' in kw)      # with_noise keeps the vector


# ---- the host rules at d + 2 parameters ----------------------------------------------------------------------------------
def test_sum_block_objectives_with_ard_gradients():
    d = 3
    base = np.arange(1.0, d + 3.0)

    def evaluate(l):
        if l == 1:
            raise np.linalg.LinAlgError('Matrix is not positive definite')
        return 10.0 ** l, base * 10.0 ** l

    lml, grad, failure = Hyper.sum_block_objectives([0, 2], evaluate)
    assert lml == 101.0 and grad.shape == (d + 2,) and np.array_equal(grad, base * 101.0) and failure == 0.0
    lml, grad, failure = Hyper.sum_block_objectives(range(3), evaluate)
    assert lml == 101.0 and np.array_equal(grad, base * 101.0) and failure == 1.0
    # no block gave a gradient: zeros of the asked length, 3 by default as ever
    lml, grad, failure = Hyper.sum_block_objectives([1], evaluate, d + 2)
    assert lml == 0.0 and np.array_equal(grad, np.zeros(d + 2)) and failure == 1.0
    assert np.array_equal(Hyper.sum_block_objectives([], evaluate)[1], np.zeros(3))
    assert np.array_equal(Hyper.sum_block_objectives([1], evaluate)[1], np.zeros(3))


def test_theta_round_trip_of_a_model_layer():
    k0 = ca.DenseMaternKernel(1.5, l=[0.5, 2.0], sf=1.3)
    theta = Hyper.pack_theta(k0.sf, k0.l, 0.01 * k0.sf)
    assert theta.shape == (4,) and np.allclose(theta, np.log([1.3, 0.5, 2.0, 0.013]), rtol=0, atol=0)
    ell, sf, noise = Hyper.unpack_theta(theta, len(k0.l))
    k = k0.with_values(ell, sf, noise)
    assert k.ard and type(k) is type(k0) and k.nu == 1.5
    np.testing.assert_allclose(k.l, k0.l, rtol=1e-15)
    np.testing.assert_allclose([k.sf, k.noise], [1.3, 0.013], rtol=1e-15)
    assert Hyper.pack_theta(k.sf, k.l, k.noise).shape == (4,)
    # the all-reduce buffer of MRGP._layer_objective, [lml | grad | failure], split from both ends whatever the width
    for grad in (np.array([1.0, 2.0, 3.0]), np.arange(1.0, 6.0)):
        vals = np.array([7.0] + list(grad) + [0.0])
        assert vals[0] == 7.0 and np.array_equal(vals[1:-1], grad) and vals[-1] == 0.0
    iso = ca.RBFKernel(l=0.7).with_values(*Hyper.unpack_theta(Hyper.pack_theta(1.0, 0.7, 0.01)))
    assert type(iso.l) is float and iso.ard is False
