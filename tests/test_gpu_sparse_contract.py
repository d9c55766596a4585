"""The memory footprint of include/cimrgp_sparse.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py): padding
columns and rows >= n of A poisoned, guards around C, g, the scratch and every other output, the strict upper triangle
of C preset and found unchanged, const inputs keep their bytes; results bit-equal to a clean run and held to NumPy."""
import numpy as np
import pytest

import sparse_numpy as sn
from test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec,
                                      _round, _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def _a_buf(name, a, tdt, extra_rows=5):
    """A (rows x m) CONST inside a wider pitch with rows below it: padding columns and those rows UNTOUCHED (poisoned)."""
    rows, m = a.shape
    ld = wide_ld(m)
    return Guarded(name, (rows + extra_rows) * ld, tdt, CUDA, ld=ld).mark(CONST, rows, m, values=a)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,q", [(1, 1, 0), (37, 16, 1), (300, 130, 3), (2049, 257, 8), (5000, 1000, 2), (777, 1025, 0)])
def test_wsyrk_tn_footprint(dev, dt, n, m, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m + q)
    a = _round(rng.normal(size=(n, m)), tdt)
    w = _round(10.0 ** rng.uniform(-2, 2, size=n), tdt)
    r = _round(rng.normal(size=(n, max(q, 1))), tdt)
    c0 = _round(rng.normal(size=(m, m)), tdt)
    ab = _a_buf("A", a, tdt)
    wb = _const_vec("w", w, tdt)
    rb = _const_vec("r", r, tdt)
    ldc = wide_ld(m)
    # lower triangle OUT (its old contents are not read); the strict upper triangle keeps its preset values
    cb = Guarded("C", (m + 3) * ldc, tdt, CUDA, ld=ldc).mark(CONST, m, m, part="upper", values=c0).mark(OUT, m, m, part="lower")
    gb = _out_vec("g", max(m * q, 1), tdt) if q else None
    lib = _lib().load()
    nbytes = int(lib.cimrgp_wsyrk_tn_scratch_bytes(_dt(tdt), n, m, q))
    assert nbytes == sn.scratch_bytes(ab.esz, n, m, q)
    scratch = Guarded("scratch", nbytes // ab.esz, tdt, CUDA).vec(JUNK, nbytes // ab.esz)
    bufs = [ab, wb, rb, cb, scratch] + ([gb] if q else [])
    run_contract(bufs, lambda: _call(lib.cimrgp_wsyrk_tn(_dt(tdt), ab.ptr(), n, m, ab.ld, wb.ptr(), rb.ptr() if q else None, q, 0.75,
                                                         cb.ptr(), ldc, gb.ptr() if q else None, scratch.ptr(), nbytes, _stream()),
                                     "cimrgp_wsyrk_tn"), _sync)
    c_ref, g_ref, bc, bg = sn.wsyrk(a, w, r[:, :q] if q else None, diag_add=0.75)
    got = _host(cb.mat(m, m))
    il = np.tril_indices(m)
    assert (np.abs(got - c_ref)[il] <= (n + 2) * UNIT[dt] * (bc + np.eye(m))[il]).all()
    assert np.array_equal(got[np.triu_indices(m, 1)], c0[np.triu_indices(m, 1)])
    if q:
        assert (np.abs(_host(gb.data)[:m * q].reshape(m, q) - g_ref) <= (n + 2) * UNIT[dt] * bg).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 1), (333, 70), (1030, 257)])
def test_sparse_lambda_footprint(dev, dt, mode, n, m):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m)
    a = _round(rng.normal(size=(n, m)) * 0.5 / np.sqrt(m), tdt)
    ab = _a_buf("A", a, tdt)
    lam, w = _out_vec("lam", n, tdt), _out_vec("w", n, tdt)
    sums = _out_vec("sums", 3, torch.float64)
    lib = _lib().load()
    run_contract([ab, lam, w, sums], lambda: _call(lib.cimrgp_sparse_lambda(_dt(tdt), ab.ptr(), n, m, ab.ld, 1.3, 0.02, mode, lam.ptr(),
                                                                            w.ptr(), sums.ptr(), _stream()), "cimrgp_sparse_lambda"), _sync)
    qd = (a * a).sum(axis=1)
    lam_ref = 1.3 - qd + 0.02 if mode == 0 else np.full(n, 0.02)
    tol = 1e-14 if dt == "f64" else 1e-6
    assert np.abs(_host(lam.data) - lam_ref).max() <= tol * 2
    assert np.abs(_host(w.data) * _host(lam.data) - 1).max() <= 4 * UNIT[dt]
    s = _host(sums.data)
    assert s[2] == 0 and abs(s[0] - np.log(_host(lam.data)).sum()) <= 1e-13 * np.abs(np.log(_host(lam.data))).sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ns,m,q", [(1, 1, 1), (333, 70, 3), (1030, 257, 8)])
def test_sparse_tail_footprint(dev, dt, acc, ns, m, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(ns + m + q)
    a = _round(rng.normal(size=(ns, m)) / np.sqrt(m), tdt)
    wst = _round(rng.normal(size=(ns, m)) / np.sqrt(m), tdt)
    gamma = _round(rng.normal(size=(m, q)), tdt)
    pre_m, pre_v = _round(rng.normal(size=ns * q), tdt), _round(rng.normal(size=ns), tdt)
    ab, wb, gb = _a_buf("A*", a, tdt), _a_buf("W*", wst, tdt), _const_vec("gamma", gamma, tdt)
    mean = _out_vec("mean", ns * q, tdt, pre=pre_m if acc else None)
    var = _out_vec("var", ns, tdt, pre=pre_v if acc else None)
    lib = _lib().load()
    run_contract([ab, wb, gb, mean, var],
                 lambda: _call(lib.cimrgp_sparse_tail(_dt(tdt), ab.ptr(), wb.ptr(), ns, m, ab.ld, gb.ptr(), q, 1.3, 0.25, mean.ptr(),
                                                      var.ptr(), acc, _stream()), "cimrgp_sparse_tail"), _sync)
    tol = 1e-13 if dt == "f64" else 1e-5
    mean_ref = wst @ gamma + (pre_m.reshape(ns, q) if acc else 0.0)
    var_ref = 1.55 - (a * a).sum(axis=1) + (wst * wst).sum(axis=1) + (pre_v if acc else 0.0)
    assert np.abs(_host(mean.data).reshape(ns, q) - mean_ref).max() <= tol * (1 + np.abs(mean_ref).max())
    assert np.abs(_host(var.data) - var_ref).max() <= tol * 8
