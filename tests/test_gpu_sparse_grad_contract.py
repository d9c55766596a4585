"""The memory footprint of include/cimrgp_sparse_grad.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py):
padding columns of G, V, A and Y and the rows below them poisoned, guards around every output and the scratch, const
inputs keep their bytes; results bit-equal to a clean run and held to NumPy."""
import numpy as np
import pytest

import sparse_grad_numpy as sg
from test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec,
                                      _round, _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401
from test_gpu_sparse_contract import UNIT, _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("na,nb,d,cov", [(1, 1, 1, 0), (37, 16, 2, 1), (600, 130, 3, 2), (2049, 257, 8, 3), (130, 130, 2, 0)])
def test_cov_pair_grad_footprint(dev, dt, acc, na, nb, d, cov):
    """Columns >= nb and rows >= na of G are never read (poisoned with NaN in one run), xa, xb and G keep their bytes,
    the scratch is written before it is read; with accumulate the outputs start from preset values."""
    tdt = TDT[dt]
    rng = np.random.default_rng(na + nb + d)
    xa = _round(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d), tdt)
    xb = xa if na == nb else _round(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d), tdt)
    g = _round(rng.normal(size=(na, nb)), tdt)
    pre_s, pre_db = _round(rng.normal(size=2), torch.float64), _round(rng.normal(size=(nb, d)), tdt)
    xab, xbb = _const_vec("xa", xa, tdt), _const_vec("xb", xb, tdt)
    gb = _a_buf("G", g, tdt)
    sums = _out_vec("sums", 2, torch.float64, pre=pre_s if acc else None)
    db = _out_vec("db", nb * d, tdt, pre=pre_db if acc else None)
    lib = _lib().load()
    nbytes = int(lib.cimrgp_cov_pair_grad_scratch_bytes(na, nb, d))
    assert nbytes == sg.pair_scratch_bytes(na, nb, d)
    scratch = Guarded("scratch", nbytes // 8, torch.float64, CUDA).vec(JUNK, nbytes // 8)
    run_contract([xab, xbb, gb, sums, db, scratch],
                 lambda: _call(lib.cimrgp_cov_pair_grad(_dt(tdt), cov, xab.ptr(), na, xbb.ptr(), nb, d, gb.ptr(), gb.ld, 0.7, 1.3, -2.0,
                                                        acc, sums.ptr(), db.ptr(), scratch.ptr(), nbytes, _stream()),
                               "cimrgp_cov_pair_grad"), _sync)
    (s_ref, db_ref), (s_mag, db_mag) = sg.pair_grad(xa, xb, g, cov, 0.7, 1.3, scale=-2.0)
    # (na + 2) u for the sums; the covariance's own error (measured in test_gpu_sparse_grad.py) is bounded here: the
    # exponent is at most 16.4 (RBF: d2 <= 16, l = 0.7) with a relative error of (d + 2) u <= 10 u, so k, g and dk/dlog l are
    # off by at most (164 + 6) u, taken 4 times as there
    factor = (na + 2 + 4 * 170) * UNIT[dt]
    if acc:
        s_ref, db_ref, s_mag, db_mag = s_ref + pre_s, db_ref + pre_db, s_mag + np.abs(pre_s), db_mag + np.abs(pre_db)
    assert (np.abs(_host(sums.data) - s_ref) <= factor * s_mag).all()
    assert (np.abs(_host(db.data).reshape(nb, d) - db_ref) <= factor * db_mag + 1e-300).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m,q", [(1, 1, 1), (333, 70, 3), (1030, 257, 8)])
def test_sparse_grad_rows_footprint(dev, dt, mode, n, m, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m + q)
    v = _round(rng.normal(size=(n, m)) / np.sqrt(m), tdt)
    gamma, r = _round(rng.normal(size=(m, q)), tdt), _round(rng.normal(size=(n, q)), tdt)
    w = _round(1.0 / (0.02 + rng.uniform(0, 1.3, size=n)), tdt)
    vb = _a_buf("V", v, tdt)
    gb, rb, wb = _const_vec("gamma", gamma, tdt), _const_vec("r", r, tdt), _const_vec("w", w, tdt)
    beta, t = _out_vec("beta", n * q, tdt), _out_vec("t", n, tdt)
    sums = _out_vec("sums", 2, torch.float64)
    lib = _lib().load()
    run_contract([vb, gb, rb, wb, beta, t, sums],
                 lambda: _call(lib.cimrgp_sparse_grad_rows(_dt(tdt), vb.ptr(), n, m, vb.ld, gb.ptr(), rb.ptr(), wb.ptr(), q, mode, 0.02,
                                                           beta.ptr(), t.ptr(), sums.ptr(), _stream()), "cimrgp_sparse_grad_rows"), _sync)
    beta_ref, t_ref, h_ref = sg.rows(v, gamma, r, w, mode, 0.02)
    tol = 1e-12 if dt == "f64" else 4 * UNIT[dt]
    assert np.abs(_host(beta.data).reshape(n, q) - beta_ref).max() <= tol * np.abs(beta_ref).max()
    assert np.abs(_host(t.data) - t_ref).max() <= tol * np.abs(t_ref).max()
    s = _host(sums.data)
    assert abs(s[0] - h_ref.sum()) <= tol * np.abs(h_ref).sum() and abs(s[1] - t_ref.sum()) <= tol * np.abs(t_ref).sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,q", [(1, 1, 1), (333, 70, 3), (1030, 257, 8)])
def test_sparse_grad_combine_footprint(dev, dt, n, m, q):
    """Y is read and written in place inside its pitch: its padding columns and the rows below keep their bytes."""
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m + q)
    a, y = _round(rng.normal(size=(n, m)), tdt), _round(rng.normal(size=(n, m)), tdt)
    beta, b = _round(rng.normal(size=(n, q)), tdt), _round(rng.normal(size=(m, q)), tdt)
    w, t = _round(rng.uniform(0.5, 2, size=n), tdt), _round(rng.normal(size=n), tdt)
    ab = _a_buf("A", a, tdt)
    ld = wide_ld(m)
    yb = Guarded("Y", (n + 5) * ld, tdt, CUDA, ld=ld).mark(INOUT, n, m, values=y)
    bb, b2, wb, tb = _const_vec("beta", beta, tdt), _const_vec("b", b, tdt), _const_vec("w", w, tdt), _const_vec("t", t, tdt)
    lib = _lib().load()
    run_contract([ab, yb, bb, b2, wb, tb],
                 lambda: _call(lib.cimrgp_sparse_grad_combine(_dt(tdt), ab.ptr(), ab.ld, yb.ptr(), ld, n, m, bb.ptr(), b2.ptr(), wb.ptr(),
                                                              tb.ptr(), q, _stream()), "cimrgp_sparse_grad_combine"), _sync)
    ref = sg.combine(a, y, beta, b, w, t)
    tol = 1e-12 if dt == "f64" else 4 * UNIT[dt]
    assert np.abs(_host(yb.mat(n, m)) - ref).max() <= tol * np.abs(ref).max()
