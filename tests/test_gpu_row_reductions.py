"""The kernels that sum in the fixed orders of cimrgp_amd/csrc/reduce.hpp, at the boundaries those helpers could break: the
64-column lane stride of the row walk (m = 63, 64, 65, 129), its four rows per workgroup (1, 4, 5 and 9 rows), every wave slot
and the ragged last workgroup.  The five sparse row entry points -- cimrgp_sparse_lambda, cimrgp_sparse_tail,
cimrgp_sparse_tail_grad, cimrgp_sparse_loo and cimrgp_sparse_grad_rows (the rows step of the sparse gradient) -- are held to
NumPy FP64 at the tolerances of their own tests (test_gpu_sparse_contract.py, test_gpu_sparse_post.py,
test_gpu_sparse_grad.py), to themselves on repetition, and row by row to the one-row call; the single-block gradient of the
log marginal likelihood is held to its batched twin.  These tests pin behaviour: they pass on the library before reduce.hpp
too."""
import numpy as np
import pytest

import sparse_grad_numpy as sg
import sparse_post_numpy as sp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
SF, NOISE, D = 1.3, 0.02, 2
COLS, ROWS, OUTS = (1, 63, 64, 65, 129), (1, 4, 5), (1, 8)
#: rows of a 9-row call held to the one-row call: every wave slot of a workgroup (0, 3), the next workgroup's first (4) and the
#: ragged last workgroup (8)
LONE = (0, 3, 4, 8)


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _round(a, dt):
    return np.asarray(a, dtype=np.float32 if dt == "f32" else np.float64).astype(np.float64)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(xs, ys):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", TDT[dt]).contiguous()


def _padded(ca, a, dt):
    """a (.., rows, cols) inside a NaN-filled buffer of padded pitch."""
    buf = torch.full(a.shape[:-1] + (ca.device.padded_ld(a.shape[-1]),), float("nan"), dtype=TDT[dt], device="cuda")
    buf[..., :a.shape[-1]] = _dev(a, dt)
    return buf


_CASES = {}


def _case(dt, n, m, q):
    """One set of host inputs per shape and dtype (values the dtype holds), shared by the tests."""
    key = (dt, n, m, q)
    if key not in _CASES:
        rng = np.random.default_rng([n, m, q])
        c = dict(a=_round(rng.normal(size=(n, m)) * 0.5 / np.sqrt(m), dt), v=_round(rng.normal(size=(n, m)) * 0.05 / np.sqrt(m), dt),
                 wst=_round(rng.normal(size=(n, m)) / np.sqrt(m), dt), gamma=_round(rng.normal(size=(m, q)), dt),
                 r=_round(rng.normal(size=(n, q)), dt), w=_round(1.0 / (0.02 + rng.uniform(0, 1.3, size=n)), dt),
                 sa=_round(rng.normal(size=(D + 1, n, m)), dt), sw=_round(rng.normal(size=(D + 1, n, m)), dt))
        _CASES[key] = c
    return _CASES[key]


def _take(c, i):
    """The case of row i alone."""
    return {k: (v if k == "gamma" else v[:, i:i + 1] if k in ("sa", "sw") else v[i:i + 1]) for k, v in c.items()}


# ---- the five calls: each returns its per-row outputs, then its sums (if any) ------------------------------------------------
def _lambda(ca, c, dt, mode=0):
    n, m = c["a"].shape
    lam, w, sums = ca.device.sparse_lambda(_padded(ca, c["a"], dt), n, m, SF, NOISE, mode)
    return (lam, w), (sums,)


def _tail(ca, c, dt):
    n, m = c["a"].shape
    q = c["gamma"].shape[1]
    mean = torch.full((n, q), float("nan"), dtype=TDT[dt], device="cuda")
    var = torch.full((n,), float("nan"), dtype=TDT[dt], device="cuda")
    ca.device.sparse_tail(_padded(ca, c["a"], dt), _padded(ca, c["wst"], dt), n, m, _dev(c["gamma"], dt), SF, 0.25, mean, var)
    return (mean, var), ()


def _tail_grad(ca, c, dt):
    _, n, m = c["sa"].shape
    q = c["gamma"].shape[1]
    mg = torch.full((n, D, q), float("nan"), dtype=TDT[dt], device="cuda")
    vg = torch.full((n, D), float("nan"), dtype=TDT[dt], device="cuda")
    ca.device.sparse_tail_grad(_padded(ca, c["sa"], dt), _padded(ca, c["sw"], dt), n, m, _dev(c["gamma"], dt), mg, vg)
    return (mg, vg), ()


def _loo(ca, c, dt, mode=0):
    n, m = c["a"].shape
    q = c["gamma"].shape[1]
    lm = torch.full((n, q), float("nan"), dtype=TDT[dt], device="cuda")
    lv = torch.full((n,), float("nan"), dtype=TDT[dt], device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ca.device.sparse_loo(_padded(ca, c["a"], dt), _padded(ca, c["v"], dt), n, m, _dev(c["gamma"], dt), _dev(c["r"], dt), SF, NOISE, mode,
                         bad, lm, lv)
    return (lm, lv), (bad,)


def _grad_rows(ca, c, dt, mode=0):
    n, m = c["v"].shape
    beta, t, sums = ca.device.sparse_grad_rows(_padded(ca, c["v"], dt), n, m, _dev(c["gamma"], dt), _dev(c["r"], dt), _dev(c["w"], dt),
                                               mode, NOISE)
    return (beta, t), (sums,)


CALLS = {"lambda": _lambda, "tail": _tail, "tail_grad": _tail_grad, "loo": _loo, "grad_rows": _grad_rows}


def _host(t):
    return t.double().cpu().numpy()


def _twice(call, ca, c, dt, *mode):
    """The call's outputs, after a second run has given the same bits."""
    rows, sums = call(ca, c, dt, *mode)
    rows2, sums2 = call(ca, c, dt, *mode)
    torch.cuda.synchronize()
    assert _same(rows + sums, rows2 + sums2)
    return rows, sums


# ---- against NumPy FP64, at each entry point's own tolerance, and bit-equal on repetition --------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("m", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_sparse_lambda_at_the_lane_and_workgroup_boundaries(ca, dt, n, m):
    """test_sparse_lambda_footprint's bounds (FITC: the mode whose lambda takes the row sum)."""
    mode = 0
    c = _case(dt, n, m, 1)
    (lam, w), (sums,) = _twice(_lambda, ca, c, dt, mode)
    lam_ref = SF - (c["a"] * c["a"]).sum(axis=1) + NOISE
    tol = 1e-14 if dt == "f64" else 1e-6
    assert np.abs(_host(lam) - lam_ref).max() <= tol * 2
    assert np.abs(_host(w) * _host(lam) - 1).max() <= 4 * UNIT[dt]
    s = _host(sums)
    assert s[2] == 0 and abs(s[0] - np.log(_host(lam)).sum()) <= 1e-13 * np.abs(np.log(_host(lam))).sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", OUTS)
@pytest.mark.parametrize("m", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_sparse_tail_at_the_lane_and_workgroup_boundaries(ca, dt, n, m, q):
    """test_sparse_tail_footprint's bounds."""
    c = _case(dt, n, m, q)
    (mean, var), _ = _twice(_tail, ca, c, dt)
    tol = 1e-13 if dt == "f64" else 1e-5
    mean_ref = c["wst"] @ c["gamma"]
    var_ref = SF + 0.25 - (c["a"] * c["a"]).sum(axis=1) + (c["wst"] * c["wst"]).sum(axis=1)
    assert np.abs(_host(mean) - mean_ref).max() <= tol * (1 + np.abs(mean_ref).max())
    assert np.abs(_host(var) - var_ref).max() <= tol * 8


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", OUTS)
@pytest.mark.parametrize("m", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_sparse_tail_grad_at_the_lane_and_workgroup_boundaries(ca, dt, n, m, q):
    """test_sparse_tail_grad_within_the_componentwise_bound's bound: |err| <= (m + 2) u sum |terms|."""
    c = _case(dt, n, m, q)
    (mg, vg), _ = _twice(_tail_grad, ca, c, dt)
    mref, vref, mmag, vmag = sp.tail_grad(c["sa"], c["sw"], c["gamma"])
    assert (np.abs(_host(mg) - mref) <= (m + 2) * UNIT[dt] * mmag).all()
    assert (np.abs(_host(vg) - vref) <= (m + 2) * UNIT[dt] * vmag).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", OUTS)
@pytest.mark.parametrize("m", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_sparse_loo_at_the_lane_and_workgroup_boundaries(ca, dt, n, m, q):
    """test_sparse_loo_within_the_propagated_bound's bounds (FITC: the mode whose lambda takes the row sum)."""
    mode = 0
    c = _case(dt, n, m, q)
    a, v, gamma, r = c["a"], c["v"], c["gamma"], c["r"]
    (lm, lv), (bad,) = _twice(_loo, ca, c, dt, mode)
    assert int(bad.item()) == 0
    mref, vref, h, mumag, lam = sp.loo_rows(a, v, gamma, r, SF, NOISE, mode)
    u = UNIT[dt]
    qd, s, mu = (a * a).sum(axis=1), (v * v).sum(axis=1), v @ gamma
    dlam = (m + 2) * u * qd
    dh = (m + 2) * u * s / lam + h * dlam / lam
    bv = dlam / np.abs(1 - h) + lam * dh / (1 - h) ** 2 + 4 * u * np.abs(vref)
    bm = ((m + 2) * u * mumag / np.abs(1 - h)[:, None] + np.abs(r - mu) * (dh / (1 - h) ** 2)[:, None] + 4 * u * np.abs(mref))
    assert (np.abs(_host(lv) - vref) <= bv).all() and (np.abs(_host(lm) - mref) <= bm).all()


def _rel_max(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", OUTS)
@pytest.mark.parametrize("m", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_sparse_grad_rows_at_the_lane_and_workgroup_boundaries(ca, dt, n, m, q):
    """test_sparse_grad_rows_and_combine_against_numpy's tolerance: FP64 1e-12 of each output's largest magnitude (the two
    sums: of the sum of magnitudes); FP32 4 x the FP32 error of cimrgp_sparse_tail (A* = W* = V) on the same V and gamma.
    FITC: t = h, the rows' own sums."""
    mode = 0
    c = _case(dt, n, m, q)
    v, gamma = c["v"], c["gamma"]
    if dt == "f64":
        tol = 1e-12
    else:
        vb, mean, var = _padded(ca, v, dt), torch.empty((n, q), dtype=TDT[dt], device="cuda"), torch.empty(n, dtype=TDT[dt], device="cuda")
        ca.device.sparse_tail(vb, vb, n, m, _dev(gamma, dt), SF, 0.0, mean, var)
        tol = 4 * max(_rel_max(_host(mean), v @ gamma), _rel_max(_host(var), np.full(n, SF)))
    (beta, t), (sums,) = _twice(_grad_rows, ca, c, dt, mode)
    beta_ref, t_ref, h_ref = sg.rows(v, gamma, c["r"], c["w"], mode, NOISE)
    sh = _host(sums)
    errs = (_rel_max(_host(beta), beta_ref), _rel_max(_host(t), t_ref), abs(sh[0] - h_ref.sum()) / np.abs(h_ref).sum(),
            abs(sh[1] - t_ref.sum()) / np.abs(t_ref).sum())
    print("grad_rows %s mode %d (%d, %d, %d): tol %.2e  beta %.2e t %.2e sum h %.2e sum t %.2e" % ((dt, mode, n, m, q, tol) + errs))
    assert max(errs) <= tol


# ---- a row's result does not depend on its place in the launch -------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_row_of_nine_equals_the_one_row_call_bit_for_bit(ca, dt, name):
    c = _case(dt, 9, 65, 3)
    rows9, _ = CALLS[name](ca, c, dt)
    for i in LONE:
        rows1, _ = CALLS[name](ca, _take(c, i), dt)
        torch.cuda.synchronize()
        assert _same([t[i:i + 1] for t in rows9], rows1), (name, i)


# ---- the single-block gradient against its batched twin ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_single_block_lml_grad_equals_the_layer_objective_at_batch_one(ca, dt):
    """cimrgp_cov_lml_grad on one block (n = 130), fed the layer call's own K^-1 and the alpha of cimrgp_potrs on the layer
    call's factor, against the gradient entries of cimrgp_layer_lml_grad_cov at batch 1.  Both finish their tile records in
    one order (lml_grad_entry, misc.hip), but the layer call's alpha comes from the rows carried through the factorisation
    and a backward solve, cimrgp_potrs' from its own forward and backward solves: MEASURED on the library before reduce.hpp
    (and the same figures after it), the two gradients are NOT bit-equal: largest gap over the largest entry 3.6e-15
    (FP64), 4.9e-8 (FP32).  So the assertion is a tolerance, from the solves' backward stability and not from those
    figures: two stable solves of K alpha = r differ by at most 2 n u cond(K) |alpha|, cond(K) <= (n sf2 + noise) / noise
    for a covariance with k(0) = sf2, and the gradient is linear in alpha alpha^T with K^-1 shared bit for bit.
    cimrgp_logdet_half on the layer call's factor is held to NumPy and to itself on repetition only: the layer call returns
    the log-determinant inside the log marginal likelihood, beside the data fit, and the ABI exposes neither term on its
    own, so that comparison is left out."""
    dev, tdt = ca.device, TDT[dt]
    n, d, q, ell, sf2, noise = 130, 2, 2, 0.7, 1.3, 0.05
    rng = np.random.default_rng(130)
    xn = rng.uniform(-2, 2, size=(n, d))
    yn = np.stack([np.sin(2 * xn[:, 0] + c) + 0.3 * xn[:, -1] for c in range(q)], axis=1) + 0.1 * rng.normal(size=(n, q)) + 0.5
    x, y = _dev(xn, dt), _dev(yn, dt)
    ws_bytes = max((dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16, 16)
    karena = torch.empty((1, n, dev.padded_ld(n)), dtype=tdt, device="cuda")
    kinv = torch.empty_like(karena)
    ws = torch.empty((1, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((1, 4), float("nan"), dtype=torch.float64, device="cuda")
    starts = torch.zeros(1, dtype=torch.int64, device="cuda")
    dev.layer_lml_grad(x, y, None, starts, n, ell, sf2, noise, None, karena, kinv, ws, info, out)
    assert int(info.item()) == 0
    # the single-block route: bias = the column means, alpha = K^-1 (y - bias) through the layer call's factor
    stats = dev.block_stats(y, None)
    alpha = dev.residual(y, None, stats[:q].contiguous())
    dev.potrs(karena[0], n, ws[0], alpha)
    g1 = dev.lml_grad(x, kinv[0], n, alpha, ell, sf2, noise)
    g2 = dev.lml_grad(x, kinv[0], n, alpha, ell, sf2, noise)
    h1, h2 = dev.logdet_half(karena[0], n), dev.logdet_half(karena[0], n)
    torch.cuda.synchronize()
    assert _same([g1, h1], [g2, h2])
    gl, gs = out[0, 1:].cpu().numpy(), g1.cpu().numpy()
    gap = float(np.abs(gl - gs).max() / np.abs(gl).max())
    print("lml_grad twin %s: layer %s single %s  gap %.3e  bit-equal %s" % (dt, gl, gs, gap, np.array_equal(gl, gs)))
    diag = np.diagonal(_host(karena[0])[:, :n])
    assert abs(float(h1.item()) - np.log(diag).sum()) <= 1e-13 * np.abs(np.log(diag)).sum()
    assert gap <= 2 * n * UNIT[dt] * (n * sf2 + noise) / noise
