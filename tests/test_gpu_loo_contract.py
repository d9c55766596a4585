"""The memory footprint of include/cimrgp_loo.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py): guards
around u, scratch, diag_out, mean_out and var_out; the strict upper triangle of L, its padding columns and the columns of
u left of r0 poisoned; const inputs keep their bytes; results bit-equal to a clean run and held to NumPy."""
import numpy as np
import pytest

from loo_numpy import kinv_diag, rel, trtri
from test_gpu_buffer_contract import (CONST, CUDA, JUNK, OUT, TDT, UNTOUCHED, Guarded, _call, _const_factor, _const_vec, _dt,
                                      _factored, _host, _lib, _out_vec, _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = {"f64": 1e-9, "f32": 5e-3}


def _const_ws(wsv, tdt):
    return Guarded("workspace", wsv.numel(), tdt, CUDA).vec(CONST, wsv.numel(), values=wsv)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,r0,m", [(65, 0, 65), (700, 0, 700), (700, 256, 300), (1025, 512, 513), (1025, 1024, 1)])
def test_trtri_rows_footprint(dev, dt, n, r0, m):
    tdt = TDT[dt]
    _, lower, wsv = _factored(dev, n, tdt, n + r0)
    lgpu = lower.double().cpu().numpy()
    lb, ws = _const_factor(lower, n, tdt), _const_ws(wsv, tdt)
    ld = wide_ld(n)
    u = Guarded("u", (m + 3) * ld, tdt, CUDA, ld=ld)
    written = torch.zeros((m, n), dtype=torch.bool)
    written[:, r0:] = True
    u.mark(OUT, m, n, part=written)                      # columns left of r0, padding and guard rows: UNTOUCHED
    lib = _lib().load()
    run_contract([lb, ws, u], lambda: _call(lib.cimrgp_trtri_rows(_dt(tdt), lb.ptr(), n, lb.ld, ws.ptr(), r0, m, u.ptr(), u.ld,
                                                                  _stream()), "cimrgp_trtri_rows"), _sync)
    want = trtri(lgpu)[r0:r0 + m, r0:]
    got = _host(u.mat(m, n))[:, r0:]
    assert rel(got, want) < TOL[dt]
    assert (got[np.tril_indices(m, -1)] == 0).all() if m > 1 else True


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,strip", [(65, 256), (700, 256), (700, 512), (1025, 256)])
def test_kinv_diag_footprint(dev, dt, n, strip):
    """Scratch of exactly cimrgp_kinv_diag_scratch_bytes(n, strip) bytes between guards."""
    tdt = TDT[dt]
    _, lower, wsv = _factored(dev, n, tdt, 2 * n + strip)
    lgpu = lower.double().cpu().numpy()
    lb, ws = _const_factor(lower, n, tdt), _const_ws(wsv, tdt)
    lib = _lib().load()
    nbytes = int(lib.cimrgp_kinv_diag_scratch_bytes(_dt(tdt), n, strip))
    esz = lb.esz
    scratch = Guarded("scratch", nbytes // esz, tdt, CUDA).vec(JUNK, nbytes // esz)
    out = _out_vec("diag_out", n, tdt)
    run_contract([lb, ws, scratch, out], lambda: _call(lib.cimrgp_kinv_diag(_dt(tdt), lb.ptr(), n, lb.ld, ws.ptr(), scratch.ptr(),
                                                                            nbytes, out.ptr(), _stream()), "cimrgp_kinv_diag"), _sync)
    assert rel(_host(out.data) / kinv_diag(lgpu), np.ones(n)) < TOL[dt]


def test_kinv_diag_batched_footprint(dev):
    """Batch 3, n = 600: factors and workspaces at strides with gaps (poisoned, unread), scratch of exactly batch strips."""
    tdt, n, batch = torch.float64, 600, 3
    lib = _lib().load()
    ld = wide_ld(n)
    l_stride = (n + 5) * ld
    larena = Guarded("L arena", batch * l_stride, tdt, CUDA, ld=ld)
    wsbytes = (int(lib.cimrgp_potrf_workspace_bytes(_dt(tdt), n)) + 15) // 16 * 16
    ws_stride = wsbytes + 64
    wsa = Guarded("workspace arena", batch * ws_stride // 8, tdt, CUDA)
    want = []
    for b in range(batch):
        _, lower, wsv = _factored(dev, n, tdt, 50 + b)
        larena.mark(CONST, n, n, off=b * l_stride, part="lower", values=lower)
        wsa.mark(CONST, 1, wsv.numel(), ld=wsv.numel(), off=b * ws_stride // 8, values=wsv)
        want.append(kinv_diag(lower.double().cpu().numpy()))
    nbytes = batch * int(lib.cimrgp_kinv_diag_scratch_bytes(_dt(tdt), n, 256))
    scratch = Guarded("scratch", nbytes // 8, tdt, CUDA).vec(JUNK, nbytes // 8)
    out = _out_vec("diag_out", batch * n, tdt)
    run_contract([larena, wsa, scratch, out],
                 lambda: _call(lib.cimrgp_kinv_diag_batched(_dt(tdt), larena.ptr(), n, ld, l_stride, wsa.ptr(), ws_stride, scratch.ptr(),
                                                            nbytes, out.ptr(), batch, _stream()), "cimrgp_kinv_diag_batched"), _sync)
    assert rel(_host(out.data).reshape(batch, n) / np.stack(want), np.ones((batch, n))) < 1e-9


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, 3, 8])
def test_loo_tail_footprint(dev, dt, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(q)
    lib = _lib().load()
    n, batch, lead, gap = 333, 3, 7, 5
    rows = lead + batch * (n + gap)
    starts_h = np.array([lead + b * (n + gap) for b in range(batch)], dtype=np.int64)
    y = np.asarray(rng.normal(size=(rows, q)), dtype=np.float32 if dt == "f32" else np.float64).astype(np.float64)
    alpha = np.asarray(rng.normal(size=(batch, n, q)), dtype=np.float32 if dt == "f32" else np.float64).astype(np.float64)
    d = np.asarray(rng.uniform(0.5, 2.0, size=(batch, n)), dtype=np.float32 if dt == "f32" else np.float64).astype(np.float64)
    yb, ab, db = _const_vec("y", y, tdt), _const_vec("alpha", alpha, tdt), _const_vec("diag", d, tdt)
    starts = Guarded("starts", batch, torch.int64, CUDA).vec(CONST, batch, values=starts_h)
    block_rows = torch.zeros(rows, dtype=torch.bool)
    for s in starts_h:
        block_rows[int(s):int(s) + n] = True
    mean = Guarded("mean_out", rows * q, tdt, CUDA, ld=q).mark(OUT, rows, q, part=block_rows[:, None].expand(rows, q))
    var = Guarded("var_out", rows, tdt, CUDA, ld=1).mark(OUT, rows, 1, part=block_rows[:, None])
    run_contract([yb, ab, db, starts, mean, var],
                 lambda: _call(lib.cimrgp_loo_batched(_dt(tdt), yb.ptr(), starts.ptr(), ab.ptr(), db.ptr(), n, q, batch, mean.ptr(),
                                                      var.ptr(), _stream()), "cimrgp_loo_batched"), _sync)
    tol = 1e-14 if dt == "f64" else 1e-6
    for b, s in enumerate(starts_h):
        s = int(s)
        assert rel(_host(mean.mat(rows, q))[s:s + n], y[s:s + n] - alpha[b] / d[b][:, None]) < tol
        assert rel(_host(var.data)[s:s + n], 1 / d[b]) < tol
    # the single-block form on block 0's rows
    m1, v1 = _out_vec("mean_out", n * q, tdt), _out_vec("var_out", n, tdt)
    y0 = _const_vec("y", y[starts_h[0]:starts_h[0] + n], tdt)
    a0, d0 = _const_vec("alpha", alpha[0], tdt), _const_vec("diag", d[0], tdt)
    run_contract([y0, a0, d0, m1, v1], lambda: _call(lib.cimrgp_loo(_dt(tdt), y0.ptr(), a0.ptr(), d0.ptr(), n, q, m1.ptr(), v1.ptr(),
                                                                    _stream()), "cimrgp_loo"), _sync)
    assert rel(_host(m1.data).reshape(n, q), y[starts_h[0]:starts_h[0] + n] - alpha[0] / d[0][:, None]) < tol
