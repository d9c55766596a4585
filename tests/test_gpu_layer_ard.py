"""The batched layer objective with one length-scale per input dimension (cimrgp_layer_lml_grad_ard_cov,
include/cimrgp_layer_ard.h) against NumPy / SciPy (tests/layer_ard_numpy.py), the isotropic twin, central differences and
FP32, at the bars of tests/test_gpu_layer_lml.py."""
import numpy as np
import pytest

import layer_ard_numpy as la
from layer_ard_numpy import COVS, rel as _rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _ells(d):
    return np.linspace(0.5, 1.6, d) if d > 1 else np.array([0.7])       # distinct per dimension


def _layer(rng, batch, n, d, q, gap=3, lead=5):
    """Blocks separated by gap rows, as in tests/test_gpu_layer_lml.py."""
    rows = lead + batch * (n + gap)
    x = rng.uniform(-2, 2, size=(rows, d))
    y = np.stack([np.sin(2 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(q)], axis=1) + 0.1 * rng.normal(size=(rows, q)) + 0.5
    fbar = 0.3 * rng.normal(size=(rows, q))
    starts = [lead + b * (n + gap) for b in range(batch)]
    return x, y, fbar, starts


def _arenas(ca, batch, n, width, dtype):
    dev = ca.device
    ld = dev.padded_ld(n)
    ws_bytes = max((dev.potrf_workspace_bytes(n, dtype) + 15) // 16 * 16, 16)
    karena = torch.empty((batch, n, ld), dtype=dtype, device="cuda")
    kinv = torch.empty((batch, n, ld), dtype=dtype, device="cuda")
    ws = torch.empty((batch, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((batch, width), np.nan, dtype=torch.float64, device="cuda")
    return karena, kinv, ws, info, out


def _run(ca, x, y, fbar, starts, n, cov, ells, sf2, noise, shared_bias=None, dtype=torch.float64):
    """The ARD call on x / ells (scaled here in FP64, as the caller of the C entry point does)."""
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
    d = x.shape[1]
    karena, kinv, ws, info, out = _arenas(ca, len(starts), n, d + 3, dtype)
    st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    ca.device.layer_lml_grad_ard(t(x * (1.0 / np.asarray(ells))), t(y), t(fbar), st, n, sf2, noise, t(shared_bias), karena, kinv, ws,
                                 info, out, cov=cov)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def _run_iso(ca, x, y, fbar, starts, n, cov, ell, sf2, noise, shared_bias=None):
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    karena, kinv, ws, info, out = _arenas(ca, len(starts), n, 4, torch.float64)
    st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    ca.device.layer_lml_grad(t(x), t(y), t(fbar), st, n, ell, sf2, noise, t(shared_bias), karena, kinv, ws, info, out, cov=cov)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def _want(x, y, fbar, starts, n, cov, ells, sf2, noise, shared_bias=None):
    res = []
    for s in starts:
        r = y[s:s + n] - (0.0 if fbar is None else fbar[s:s + n])
        r = r - (r.mean(axis=0) if shared_bias is None else shared_bias)
        lml, g = la.lml_grad(x[s:s + n], r, cov, ells, sf2, noise)
        res.append([lml] + list(g))
    return np.asarray(res)


CASES = [  # batch, n, d, q, with fbar, shared bias
    (1, 65, 1, 2, True, False),        # one tile plus a row
    (3, 256, 2, 3, False, True),
    (5, 300, 3, 3, True, True),        # ragged; d = 3 takes with_dim's run-time arm
    (3, 1025, 2, 2, True, False),      # crosses four panels
    (2, 65, 8, 2, False, False),       # d = MAXD
]


@pytest.mark.parametrize("batch,n,d,q,with_fbar,shared", CASES)
def test_layer_lml_grad_ard_matches_numpy(ca, batch, n, d, q, with_fbar, shared):
    rng = np.random.default_rng(1000 * batch + n + d)
    x, y, fbar, starts = _layer(rng, batch, n, d, q)
    fbar = fbar if with_fbar else None
    sb = np.array([0.4, -0.2, 0.1][:q]) if shared else None
    ells = _ells(d)
    for cov in COVS:
        got, info = _run(ca, x, y, fbar, starts, n, cov, ells, 1.3, 0.05, sb)
        want = _want(x, y, fbar, starts, n, cov, ells, 1.3, 0.05, sb)
        assert got.shape == (batch, d + 3) and np.all(info == 0), (cov, info)
        print("cov %d: lml gap %.3e, gradient gaps %s" % (cov, np.max(np.abs(got[:, 0] - want[:, 0]) / np.abs(want[:, 0])),
                                                         ["%.2e" % _rel(got[b, 1:], want[b, 1:]) for b in range(batch)]))
        assert np.max(np.abs(got[:, 0] - want[:, 0]) / np.abs(want[:, 0])) < 1e-9, cov
        for b in range(batch):
            assert _rel(got[b, 1:], want[b, 1:]) < 1e-7, (cov, b)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_equal_length_scales_give_the_isotropic_call(ca, d):
    rng = np.random.default_rng(40 + d)
    n, ell = 300, 0.7
    x, y, fbar, starts = _layer(rng, 3, n, d, 2)
    for cov in COVS:
        ard, info = _run(ca, x, y, fbar, starts, n, cov, np.full(d, ell), 1.3, 0.05)
        iso, info_iso = _run_iso(ca, x, y, fbar, starts, n, cov, ell, 1.3, 0.05)
        assert np.all(info == 0) and np.all(info_iso == 0)
        assert np.max(np.abs(ard[:, 0] - iso[:, 0]) / np.abs(iso[:, 0])) < 1e-9, cov
        for b in range(3):
            folded = [ard[b, 1], ard[b, 2:2 + d].sum(), ard[b, d + 2]]       # sum_k d/dlog l_k = d/dlog l
            assert _rel(folded, iso[b, 1:]) < 1e-7, (cov, b)


def test_layer_lml_grad_ard_matches_finite_differences(ca):
    rng = np.random.default_rng(7)
    n, d = 200, 2
    x, y, fbar, starts = _layer(rng, 2, n, d, 2)
    th = np.log([1.1, 0.6, 1.3, 0.08])             # (sf2, l_1, l_2, noise)
    for cov in COVS:
        f = lambda t: _run(ca, x, y, fbar, starts, n, cov, np.exp(t[1:-1]), np.exp(t[0]), np.exp(t[-1]))[0]
        g = f(th)[:, 1:]
        for i in range(d + 2):
            h = 1e-5
            e = np.zeros(d + 2)
            e[i] = h
            fd = (f(th + e)[:, 0] - f(th - e)[:, 0]) / (2 * h)
            assert np.max(np.abs(fd - g[:, i]) / (np.abs(g[:, i]) + 1e-3)) < 1e-5, (cov, i)


def test_non_pd_block_leaves_the_others_intact(ca):
    rng = np.random.default_rng(3)
    n = 65
    x, y, fbar, starts = _layer(rng, 3, n, 1, 2)
    for s in starts:                               # well-spread inputs: the exponential covariance is PD without noise
        x[s:s + n, 0] = np.linspace(-2, 2, n) + 0.01 * rng.uniform(size=n)
    x[starts[1]:starts[1] + n, 0] = 0.25           # block 1: every input the same
    got, info = _run(ca, x, y, fbar, starts, n, 1, np.array([0.5]), 1.0, 0.0)
    assert info[1] > 0 and info[0] == 0 and info[2] == 0
    want = _want(x, y, fbar, [starts[0], starts[2]], n, 1, np.array([0.5]), 1.0, 0.0)
    for i, b in enumerate((0, 2)):
        assert abs(got[b, 0] - want[i, 0]) / abs(want[i, 0]) < 1e-9
        assert _rel(got[b, 1:], want[i, 1:]) < 1e-7


def test_fp32_agrees_with_fp64(ca):
    rng = np.random.default_rng(11)
    n, d = 128, 2
    x, y, fbar, starts = _layer(rng, 3, n, d, 2)
    ells = np.array([0.8, 1.3])
    for cov in COVS:
        g64, i64 = _run(ca, x, y, fbar, starts, n, cov, ells, 1.0, 0.2)
        g32, i32 = _run(ca, x, y, fbar, starts, n, cov, ells, 1.0, 0.2, dtype=torch.float32)
        assert np.all(i32 == 0) and np.all(i64 == 0)
        assert np.max(np.abs(g32[:, 0] - g64[:, 0]) / np.abs(g64[:, 0])) < 1e-3, cov
        for b in range(3):
            assert _rel(g32[b, 1:], g64[b, 1:]) < 1e-3, (cov, b)


def test_isotropic_call_is_what_it_was_beside_the_ard_call(ca):
    """The isotropic entry point shares its host steps and finishing body with the ARD one: its NumPy parity at the bars
    of tests/test_gpu_layer_lml.py, and run-to-run bit equality with an ARD call in between."""
    rng = np.random.default_rng(5)
    n = 300
    x, y, fbar, starts = _layer(rng, 3, n, 2, 2)
    first, _ = _run_iso(ca, x, y, fbar, starts, n, 2, 0.7, 1.3, 0.05)
    _run(ca, x, y, fbar, starts, n, 2, np.array([0.5, 1.6]), 1.3, 0.05)
    again, info = _run_iso(ca, x, y, fbar, starts, n, 2, 0.7, 1.3, 0.05)
    assert np.all(info == 0) and np.array_equal(first, again)
    want = _want(x, y, fbar, starts, n, 2, 0.7, 1.3, 0.05)
    assert np.max(np.abs(first[:, 0] - want[:, 0]) / np.abs(want[:, 0])) < 1e-9
    for b in range(3):
        assert _rel(first[b, 1:], want[b, 1:]) < 1e-7


def test_gram_of_an_ard_kernel_is_the_unit_gram_of_scaled_inputs(ca):
    """``K`` / ``gram`` of a kernel object with a length-scale vector: the same device call on x / l at l = 1."""
    rng = np.random.default_rng(2)
    x, x2 = rng.uniform(-2, 2, size=(70, 2)), rng.uniform(-2, 2, size=(33, 2))
    ells = np.array([0.5, 1.6])
    for cov in COVS:
        make = (lambda l: ca.RBFKernel(l=l, sf=1.3)) if cov == 0 else (lambda l: ca.DenseMaternKernel(COVS[cov], l=l, sf=1.3))
        for args, scaled in (((x,), (x * (1.0 / ells),)), ((x, x2), (x * (1.0 / ells), x2 * (1.0 / ells)))):
            got, want = make(ells).K(*args), make(1.0).K(*scaled)
            assert got.shape == want.shape and np.array_equal(got, want), cov
            oracle_k = la.cov_ard(args[0], args[-1], cov, ells, 1.3, want_grad=False)[0]
            assert _rel(np.tril(got) if len(args) == 1 else got, np.tril(oracle_k) if len(args) == 1 else oracle_k) < 1e-12, cov
