"""The buffer contract of the joint entry points (include/cimrgp_joint.h), with the helpers of
tests/test_gpu_buffer_contract.py: every buffer between guards, leading dimensions wider than padded_ld, gaps between
batched blocks, unread regions poisoned with zeros, NaN and random values in three runs.  Guards, padding, gaps and
const inputs keep their bytes (a factor's strict upper triangle poisoned with NaN included: none of it may reach the
output), outputs are bit-equal across the runs and match NumPy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, Guarded, _call, _const_vec, _dt, _host, _kcov,  # noqa: E402
                                            _lib, _rel, _round, _stream, _sync, run_contract, wide_ld)
from tests.test_joint_host import phi  # noqa: E402

TDT = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _ints(name, a):
    a = np.asarray(a, dtype=np.int64)
    return Guarded(name, a.size, torch.int64, CUDA).vec(CONST, a.size, values=a)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_normal_fill_footprint(dev, dt):
    tdt = TDT[dt]
    cols, ns, batch = 5, 131, 3
    ldz = wide_ld(ns)
    zs = (cols + 2) * ldz
    keys = [(1 << 32) + 4, 9, (3 << 32)]
    gk = _ints("keys", keys)
    z = Guarded("z", batch * zs, tdt, CUDA, ld=ldz)
    for b in range(batch):
        z.mark(OUT, cols, ns, off=b * zs)
    lib = _lib().load()
    run_contract([gk, z], lambda: _call(lib.cimrgp_normal_fill(_dt(tdt), 99, gk.ptr(), batch, 2, cols, ns, z.ptr(), ldz, zs,
                                                               _stream()), "cimrgp_normal_fill"), _sync)
    for b in range(batch):
        got = _host(z.mat(cols, ns, off=b * zs))
        assert _rel(got, phi(99, keys[b], cols, ns, col0=2)) < (1e-6 if dt == "f32" else 1e-14)


def _factored_blocks(dev, tdt, n, batch, ldl, ls, cov, ell, sf2, noise, x, starts):
    """L_b and the workspace of each block (device potrf), as host arrays for CONST buffers."""
    lh, wsh = [], []
    for b in range(batch):
        xb = torch.tensor(x[starts[b]:starts[b] + n], dtype=tdt, device=CUDA)
        k = dev.rbf_gram(xb, ell, sf2, noise, lower_only=True, cov=cov)
        ws, info = dev.potrf(k, n)
        assert int(info.item()) == 0
        lh.append(np.tril(_host(k[:, :n])))
        wsh.append(ws.cpu().numpy())
    return lh, wsh


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("factor", [False, True])
def test_layer_joint_cov_footprint(dev, dt, factor):
    tdt = TDT[dt]
    n, ns, d, batch, cov = 300, 70, 2, 2, 2
    ell, sf2, noise = 0.6, 1.2, 0.05
    rng = np.random.default_rng(17)
    x = _round(np.sort(rng.uniform(-1.5, 1.5, size=(2 * n + 40, d)), axis=0), tdt)
    starts = [7, n + 29]
    xs = _round(rng.uniform(-1.5, 1.5, size=(2 * ns + 9, d)), tdt)
    t_starts = [4, ns + 9]
    ldl, ldw, ldc = wide_ld(n), wide_ld(n), wide_ld(ns)
    ls, wsd, cs = (n + 3) * ldl, (ns + 2) * ldw, (ns + 2) * ldc
    lh, wsh = _factored_blocks(dev, tdt, n, batch, ldl, ls, cov, ell, sf2, noise, x, starts)
    esz = torch.empty((), dtype=tdt).element_size()
    gx, gxs = _const_vec("x", x, tdt), _const_vec("xs", xs, tdt)
    gs, gts = _ints("starts", starts), _ints("t_starts", t_starts)
    gl = Guarded("L", batch * ls, tdt, CUDA, ld=ldl)
    for b in range(batch):
        gl.mark(CONST, n, n, off=b * ls, part="lower", values=lh[b])
    wsb = (wsh[0].size + 15) // 16 * 16 + 64
    gws = Guarded("ws", batch * wsb, torch.uint8, CUDA)
    for b in range(batch):
        gws.vec(CONST, wsh[b].size, off=b * wsb, values=wsh[b])
    diag = _round(np.array([1e-3, 2e-2]), tdt)
    gd = _const_vec("diag", diag, tdt)
    gw = Guarded("W", batch * wsd, tdt, CUDA, ld=ldw)
    gc = Guarded("C", batch * cs, tdt, CUDA, ld=ldc)
    for b in range(batch):
        gw.mark(JUNK, ns, n, off=b * wsd)
        if factor:
            gc.mark(OUT, ns, ns, off=b * cs)
        else:
            gc.mark(OUT, ns, ns, off=b * cs, part="lower").mark(JUNK, ns, ns, off=b * cs, part="upper")
    bufs = [gx, gxs, gs, gts, gl, gws, gd, gw, gc]
    cwsb = cws = info = None
    if factor:
        used = int(_lib().load().cimrgp_potrf_workspace_bytes(_dt(tdt), ns))
        cwsb = (used + 15) // 16 * 16 + 32
        cws = Guarded("cws", batch * cwsb // esz, tdt, CUDA)
        for b in range(batch):
            cws.vec(JUNK, (used + esz - 1) // esz, off=b * (cwsb // esz))
        info = Guarded("info", batch, torch.int32, CUDA).vec(INOUT, batch, values=np.full(batch, 0x5A5A5A5A))
        bufs += [cws, info]
    lib = _lib().load()

    def call():
        _call(lib.cimrgp_layer_joint_cov(_dt(tdt), cov, gx.ptr(), gs.ptr(), n, d, gxs.ptr(), gts.ptr(), ns, batch, ell, sf2,
                                         gl.ptr(), ldl, ls, gws.ptr(), wsb, gd.ptr(), gw.ptr(), ldw, wsd, gc.ptr(), ldc, cs,
                                         cws.ptr() if factor else None, cwsb if factor else 0,
                                         info.ptr() if factor else None, _stream()), "cimrgp_layer_joint_cov")
    run_contract(bufs, call, _sync)
    tol = 2e-3 if dt == "f32" else 1e-9
    for b in range(batch):
        xb, tb = x[starts[b]:starts[b] + n], xs[t_starts[b]:t_starts[b] + ns]
        ks = _kcov(tb, xb, cov, ell, sf2)
        want = _kcov(tb, tb, cov, ell, sf2) - ks @ np.linalg.solve(_kcov(xb, xb, cov, ell, sf2) + noise * np.eye(n), ks.T) \
            + diag[b] * np.eye(ns)
        got = _host(gc.mat(ns, ns, off=b * cs))
        if factor:
            assert np.all(np.triu(got, 1) == 0.0)
            got = got @ got.T
        assert _rel(np.tril(got), np.tril(want)) < tol, b
    if factor:
        assert list(info.data.cpu().numpy()) == [0, 0]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ns,cols", [(37, 9), (300, 200)])
def test_layer_sample_footprint(dev, dt, ns, cols):
    tdt = TDT[dt]
    batch = 2
    rng = np.random.default_rng(ns)
    ldl, ldz = wide_ld(ns), wide_ld(ns)
    ls, zs = (ns + 2) * ldl, (cols + 1) * ldz
    lh = [np.tril(_round(rng.normal(size=(ns, ns)), tdt)) for _ in range(batch)]
    zh = [_round(rng.normal(size=(cols, ns)), tdt) for _ in range(batch)]
    gl = Guarded("L", batch * ls, tdt, CUDA, ld=ldl)
    gz = Guarded("z", batch * zs, tdt, CUDA, ld=ldz)
    for b in range(batch):
        gl.mark(CONST, ns, ns, off=b * ls, part="lower", values=lh[b])    # strict upper: poisoned, must not be used
        gz.mark(CONST, cols, ns, off=b * zs, values=zh[b])
    t_starts = [3, ns + 11]
    ld_out = wide_ld(2 * ns + 20)
    pre = _round(rng.normal(size=(cols, ld_out)), tdt)
    gts = _ints("t_starts", t_starts)
    go = Guarded("out", (cols + 1) * ld_out, tdt, CUDA, ld=ld_out)
    for b in range(batch):
        go.mark(INOUT, cols, ns, off=t_starts[b], values=pre[:, t_starts[b]:t_starts[b] + ns])
    lib = _lib().load()
    run_contract([gl, gz, gts, go], lambda: _call(lib.cimrgp_layer_sample(_dt(tdt), gl.ptr(), ldl, ls, ns, batch, gz.ptr(), ldz, zs,
                                                                          cols, gts.ptr(), go.ptr(), ld_out, _stream()),
                                                  "cimrgp_layer_sample"), _sync)
    got = _host(go.mat(cols, ld_out))
    assert np.all(np.isfinite(got[:, t_starts[0]:t_starts[0] + ns]))
    for b in range(batch):
        a = t_starts[b]
        want = pre[:, a:a + ns] + zh[b] @ lh[b].T
        assert _rel(got[:, a:a + ns], want) < (1e-5 if dt == "f32" else 1e-13), b
