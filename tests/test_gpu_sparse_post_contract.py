"""The memory footprint of include/cimrgp_sparse_post.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py), in the
manner of the other *_contract.py files: padding columns (>= m) and the rows below every matrix are poisoned, point arrays end
where a guard begins, outputs sit between guards, const inputs keep their bytes, and the outputs are the same bits whatever
the poison."""
import numpy as np
import pytest

import sparse_post_numpy as sp
from test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec,
                                      _rel, _round, _stream, _sync, _ws_buf, dev, run_contract, wide_ld)  # noqa: F401
from test_gpu_sparse_contract import _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [(1, 16, 1, 1), (255, 100, 2, 2), (600, 257, 3, 2), (257, 1000, 8, 8)]
TOL = {"f64": 1e-12, "f32": 1e-4}


def _slab_buf(name, a, tdt, role, extra_rows=5):
    """(s, rows, m) slabs inside a wider pitch with rows below each slab: everything outside the s regions UNTOUCHED."""
    s, rows, m = a.shape
    ld = wide_ld(m)
    stride = (rows + extra_rows) * ld
    b = Guarded(name, s * stride, tdt, CUDA, ld=ld)
    for k in range(s):
        b.mark(role, rows, m, off=k * stride, values=a[k] if role == CONST else None)
    b.stride = stride
    return b


def _slabs_of(b, s, rows, m):
    return np.stack([_host(b.mat(rows, m, off=k * b.stride)) for k in range(s)])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_cov_cross_grad_footprint(dev, dt, ns, m, d, q):
    tdt = TDT[dt]
    cov = (ns + d) % 4
    rng = np.random.default_rng(ns + m + d)
    xa = _round(rng.uniform(-2, 2, size=(ns, d)) / np.sqrt(d), tdt)
    xb = _round(rng.uniform(-2, 2, size=(m, d)) / np.sqrt(d), tdt)
    xab, xbb = _const_vec("xa", xa, tdt), _const_vec("xb", xb, tdt)
    out = _slab_buf("out", np.zeros((d + 1, ns, m)), tdt, OUT)
    lib = _lib().load()
    run_contract([xab, xbb, out], lambda: _call(lib.cimrgp_cov_cross_grad(_dt(tdt), cov, xab.ptr(), ns, xbb.ptr(), m, d, 0.7, 1.3,
                                                                          out.ptr(), out.ld, out.stride, _stream()),
                                                "cimrgp_cov_cross_grad"), _sync)
    assert _rel(_slabs_of(out, d + 1, ns, m), sp.cross_grad(xa, xb, cov, 0.7, 1.3)) <= TOL[dt]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_tail_grad_footprint(dev, dt, acc, ns, m, d, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(ns + m + d + q)
    a, w = _round(rng.normal(size=(d + 1, ns, m)), tdt), _round(rng.normal(size=(d + 1, ns, m)), tdt)
    gamma = _round(rng.normal(size=(m, q)), tdt)
    pre_m, pre_v = _round(rng.normal(size=(ns, d, q)), tdt), _round(rng.normal(size=(ns, d)), tdt)
    ab, wb, gb = _slab_buf("A", a, tdt, CONST), _slab_buf("W", w, tdt, CONST), _const_vec("gamma", gamma, tdt)
    mg = _out_vec("mean_grad", ns * d * q, tdt, pre=pre_m if acc else None)
    vg = _out_vec("var_grad", ns * d, tdt, pre=pre_v if acc else None)
    lib = _lib().load()
    run_contract([ab, wb, gb, mg, vg], lambda: _call(lib.cimrgp_sparse_tail_grad(_dt(tdt), ab.ptr(), wb.ptr(), ns, m, d, ab.ld, ab.stride,
                                                                                gb.ptr(), q, mg.ptr(), vg.ptr(), acc, _stream()),
                                                     "cimrgp_sparse_tail_grad"), _sync)
    mref, vref, _, _ = sp.tail_grad(a, w, gamma)
    if acc:
        mref, vref = mref + pre_m, vref + pre_v
    assert _rel(_host(mg.data).reshape(ns, d, q), mref) <= TOL[dt] * m and _rel(_host(vg.data).reshape(ns, d), vref) <= TOL[dt] * m


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_loo_footprint(dev, dt, mode, ns, m, d, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(ns + m + q)
    a = _round(rng.normal(size=(ns, m)) * 0.5 / np.sqrt(m), tdt)
    v = _round(rng.normal(size=(ns, m)) * 0.05 / np.sqrt(m), tdt)
    gamma, r = _round(rng.normal(size=(m, q)), tdt), _round(rng.normal(size=(ns, q)), tdt)
    ab, vb = _a_buf("A", a, tdt), _a_buf("V", v, tdt)
    gb, rb = _const_vec("gamma", gamma, tdt), _const_vec("r", r, tdt)
    lm, lv = _out_vec("loo_mean", ns * q, tdt), _out_vec("loo_var", ns, tdt)
    bad = Guarded("bad", 1, torch.int32, CUDA).vec(INOUT, 1, values=np.full(1, 5, dtype=np.int64))
    lib = _lib().load()
    run_contract([ab, vb, gb, rb, lm, lv, bad],
                 lambda: _call(lib.cimrgp_sparse_loo(_dt(tdt), ab.ptr(), vb.ptr(), ns, m, ab.ld, gb.ptr(), rb.ptr(), q, 1.3, 0.02, mode,
                                                     lm.ptr(), lv.ptr(), bad.ptr(), _stream()), "cimrgp_sparse_loo"), _sync)
    mref, vref, h, _, _ = sp.loo_rows(a, v, gamma, r, 1.3, 0.02, mode)
    assert h.max() < 0.9 and int(bad.data[0].item()) == 5                  # no bad row: the count keeps its value
    assert _rel(_host(lm.data).reshape(ns, q), mref) <= TOL[dt] * 10 and _rel(_host(lv.data), vref) <= TOL[dt] * 10


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("factor", [0, 1])
@pytest.mark.parametrize("ns,m,d,q", SHAPES)
def test_sparse_joint_cov_footprint(dev, dt, factor, ns, m, d, q):
    """Without a workspace: the lower triangle is the output, the strict upper triangle of C (poisoned) is never used -- the
    Gram's tiles that hold the diagonal may write into it (JUNK), as cimrgp_cov_gram's lower_only does.  With one: L in the
    lower triangle, zeros above it, info set."""
    tdt = TDT[dt]
    cov = (ns + d) % 4
    rng = np.random.default_rng(ns + m + d + factor)
    xs = _round(rng.uniform(-2, 2, size=(ns, d)) / np.sqrt(d), tdt)
    a = _round(rng.normal(size=(ns, m)) * 0.1 / np.sqrt(m), tdt)
    w = _round(rng.normal(size=(ns, m)) / np.sqrt(m), tdt)
    xb, ab, wb = _const_vec("xs", xs, tdt), _a_buf("A*", a, tdt), _a_buf("W*", w, tdt)
    ldc = wide_ld(ns)
    cb = Guarded("C", (ns + 3) * ldc, tdt, CUDA, ld=ldc)
    lib = _lib().load()
    if factor:
        cb.mark(OUT, ns, ns)
        ws = _ws_buf(ns, tdt)
        info = Guarded("info", 1, torch.int32, CUDA).vec(INOUT, 1, values=np.full(1, 0x5A5A5A5A, dtype=np.int64))
        bufs = [xb, ab, wb, cb, ws, info]
        args = (ws.ptr(), ws.nbytes, info.ptr())
    else:
        cb.mark(OUT, ns, ns, part="lower").mark(JUNK, ns, ns, part="upper")
        bufs = [xb, ab, wb, cb]
        args = (None, 0, None)
    run_contract(bufs, lambda: _call(lib.cimrgp_sparse_joint_cov(_dt(tdt), cov, xb.ptr(), ns, d, 0.7, 1.3, 1.0, ab.ptr(), wb.ptr(), m,
                                                                 ab.ld, cb.ptr(), ldc, args[0], args[1], args[2], _stream()),
                                     "cimrgp_sparse_joint_cov"), _sync)
    ref = sp.kcov(xs, xs, cov, 0.7, 1.3) + np.eye(ns) - a @ a.T + w @ w.T
    got = _host(cb.mat(ns, ns))
    if factor:
        assert int(info.data[0].item()) == 0 and (got[np.triu_indices(ns, 1)] == 0).all()
        assert _rel(got @ got.T, ref) <= TOL[dt] * 10
    else:
        assert _rel(np.tril(got), np.tril(ref)) <= TOL[dt] * 10
