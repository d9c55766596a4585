"""The two calls of include/cimrgp_sparse_layer.h in the manner of tests/test_gpu_sparse_contract.py (Guarded / run_contract of
tests/test_gpu_buffer_contract.py): padding columns and rows >= n poisoned with NaN and never read, guards around every
buffer, const inputs keep their bytes; and each call bit-equal to its twin of include/cimrgp_sparse.h on the same values."""
import numpy as np
import pytest

from test_gpu_buffer_contract import (CONST, CUDA, TDT, _call, _const_vec, _dt, _host, _ints, _lib, _out_vec, _round, _stream, _sync,
                                      dev, run_contract)  # noqa: F401
from test_gpu_sparse_contract import _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SF2, NOISE = 1.3, 0.02


def _outputs(bufs):
    return [_ints(b.outputs()).clone() for b in bufs]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 16), (255, 100), (4097, 130)])
def test_sparse_lambda_dev_footprint_and_bit_equality(dev, dt, mode, n, m):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m)
    a = _round(rng.normal(size=(n, m)) * 0.5 / np.sqrt(m), tdt)
    noise = _round(np.array([NOISE]), tdt)                          # the value as the device holds it
    ab, nb = _a_buf("A", a, tdt), _const_vec("noise", noise, tdt)
    lam, w = _out_vec("lam", n, tdt), _out_vec("w", n, tdt)
    sums = _out_vec("sums", 3, torch.float64)
    lib = _lib().load()
    bufs = [ab, nb, lam, w, sums]
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_lambda_dev(_dt(tdt), ab.ptr(), n, m, ab.ld, SF2, nb.ptr(), mode, lam.ptr(),
                                                                  w.ptr(), sums.ptr(), _stream()), "cimrgp_sparse_lambda_dev"), _sync)
    got = _outputs(bufs)
    qd = (a * a).sum(axis=1)
    lam_ref = SF2 - qd + noise[0] if mode == 0 else np.full(n, noise[0])
    assert np.abs(_host(lam.data) - lam_ref).max() <= (1e-14 if dt == "f64" else 1e-6) * 2
    assert _host(sums.data)[2] == 0
    # the twin with the same noise value as a host number
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_lambda(_dt(tdt), ab.ptr(), n, m, ab.ld, SF2, float(noise[0]), mode, lam.ptr(),
                                                              w.ptr(), sums.ptr(), _stream()), "cimrgp_sparse_lambda"), _sync)
    for b, x, y in zip(bufs, got, _outputs(bufs)):
        assert torch.equal(x, y), b.name


def _tail_problem(ns, m, q, tdt, acc):
    rng = np.random.default_rng(ns + m + q)
    a = _round(rng.normal(size=(ns, m)) / np.sqrt(m), tdt)
    wst = _round(rng.normal(size=(ns, m)) / np.sqrt(m), tdt)
    gamma = _round(rng.normal(size=(m, q)), tdt)
    bias = _round(rng.normal(size=q), tdt)
    extra = _round(np.array([0.0625 + 1e-3]), tdt)
    pre_m, pre_v = _round(rng.normal(size=ns * q), tdt), _round(rng.normal(size=ns), tdt)
    bufs = dict(a=_a_buf("A*", a, tdt), w=_a_buf("W*", wst, tdt), gamma=_const_vec("gamma", gamma, tdt),
                bias=_const_vec("bias", bias, tdt), extra=_const_vec("extra", extra, tdt),
                mean=_out_vec("mean", ns * q, tdt, pre=pre_m if acc else None),
                var=_out_vec("var", ns, tdt, pre=pre_v if acc else None))
    return (a, wst, gamma, bias, extra, pre_m, pre_v), bufs


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ns,m,q", [(1, 16, 1), (255, 100, 3), (1030, 130, 8)])
def test_sparse_tail_dev_footprint_and_values(dev, dt, acc, ns, m, q):
    tdt = TDT[dt]
    (a, wst, gamma, bias, extra, pre_m, pre_v), b = _tail_problem(ns, m, q, tdt, acc)
    lib = _lib().load()
    bufs = list(b.values())
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_tail_dev(_dt(tdt), b["a"].ptr(), b["w"].ptr(), ns, m, b["a"].ld, b["gamma"].ptr(),
                                                                q, SF2, 0.25, b["bias"].ptr(), b["extra"].ptr(), b["mean"].ptr(),
                                                                b["var"].ptr(), acc, _stream()), "cimrgp_sparse_tail_dev"), _sync)
    tol = 1e-13 if dt == "f64" else 1e-5
    mean_ref = wst @ gamma + bias + (pre_m.reshape(ns, q) if acc else 0.0)
    var_ref = SF2 + 0.25 + extra[0] - (a * a).sum(axis=1) + (wst * wst).sum(axis=1) + (pre_v if acc else 0.0)
    assert np.abs(_host(b["mean"].data).reshape(ns, q) - mean_ref).max() <= tol * (1 + np.abs(mean_ref).max())
    assert np.abs(_host(b["var"].data) - var_ref).max() <= tol * 8
    # the mean alone needs neither A* nor the extra variance, the variance alone neither gamma nor the bias
    mean_all = _ints(b["mean"].outputs()).clone()
    run_contract([b["w"], b["gamma"], b["bias"], b["mean"]],
                 lambda: _call(lib.cimrgp_sparse_tail_dev(_dt(tdt), None, b["w"].ptr(), ns, m, b["w"].ld, b["gamma"].ptr(), q, SF2, 0.25,
                                                          b["bias"].ptr(), None, b["mean"].ptr(), None, acc, _stream()),
                               "cimrgp_sparse_tail_dev"), _sync)
    assert torch.equal(mean_all, _ints(b["mean"].outputs()))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ns,m,q", [(1, 16, 1), (255, 100, 3), (1030, 130, 8)])
def test_sparse_tail_dev_without_the_new_inputs_is_sparse_tail(dev, dt, acc, ns, m, q):
    tdt = TDT[dt]
    _, b = _tail_problem(ns, m, q, tdt, acc)
    lib = _lib().load()
    bufs = [b[k] for k in ("a", "w", "gamma", "mean", "var")]
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_tail_dev(_dt(tdt), b["a"].ptr(), b["w"].ptr(), ns, m, b["a"].ld, b["gamma"].ptr(),
                                                                q, SF2, 0.25, None, None, b["mean"].ptr(), b["var"].ptr(), acc,
                                                                _stream()), "cimrgp_sparse_tail_dev"), _sync)
    got = _outputs(bufs)
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_tail(_dt(tdt), b["a"].ptr(), b["w"].ptr(), ns, m, b["a"].ld, b["gamma"].ptr(), q,
                                                            SF2, 0.25, b["mean"].ptr(), b["var"].ptr(), acc, _stream()),
                                     "cimrgp_sparse_tail"), _sync)
    for buf, x, y in zip(bufs, got, _outputs(bufs)):
        assert torch.equal(x, y), buf.name
