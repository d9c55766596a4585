"""GPU tests of the predictive gradients (include/cimrgp_grad.h): the backward row solve against NumPy, the fused
contraction against the NumPy restatement (tests/grad_numpy.py), the model's and the plugin's predictive_gradients
against central differences of their own predictions and a NumPy build from the fitted blocks, and the buffer footprint
of the new entry points (Guarded / run_contract of tests/test_gpu_buffer_contract.py)."""
import numpy as np
import pytest
import scipy.linalg as sla

from grad_numpy import central_diff, contract, kcov, rel
from test_gpu_buffer_contract import CONST, INOUT, JUNK, OUT, Guarded, run_contract, wide_ld

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _factor(dev, n, tdt, seed, cov=0, ell=0.8, noise=0.5, d=2):
    """A device factor of K = k(x, x) + noise I: (x, K, lbuf, ws, L on the host)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d))
    K = kcov(x, x, cov, ell, 1.0) + noise * np.eye(n)
    kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
    kbuf[:n, :n] = torch.as_tensor(K, dtype=tdt)
    ws, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    L = np.tril(kbuf[:n, :n].double().cpu().numpy())
    return x, K, kbuf, ws, L


# ---- B <- B L^-1 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [256, 1000, 4097])
@pytest.mark.parametrize("m", [1, 37, 1024])
def test_trsm_rows_lt_matches_numpy(dev, dt, n, m):
    tdt = TDT[dt]
    _, _, kbuf, ws, L = _factor(dev, n, tdt, seed=n + m)
    rng = np.random.default_rng(m)
    B = rng.normal(size=(m, n))
    bbuf = dev.alloc_matrix(m, n, tdt, "cuda")
    bbuf.fill_(float("nan"))                           # the padding columns are never read
    bbuf[:m, :n] = torch.as_tensor(B, dtype=tdt)
    dev.trsm_rows_lt(kbuf, n, ws, bbuf, m)
    got = bbuf[:m, :n].double().cpu().numpy()
    want = sla.solve_triangular(L, B.T, trans="T", lower=True).T          # B L^-1
    assert np.isfinite(got).all()
    assert rel(got, want) < (1e-11 if dt == "f64" else 2e-4), rel(got, want)
    assert torch.isnan(bbuf[:m, n:]).all()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [256, 1000, 4097])
def test_forward_then_backward_row_solve_gives_k_inverse_rows(dev, dt, n):
    tdt = TDT[dt]
    x, K, kbuf, ws, L = _factor(dev, n, tdt, seed=3 * n)
    xs = np.random.default_rng(1).uniform(-2, 2, size=(37, 2))
    ks = kcov(xs, x, 0, 0.8, 1.0)
    w = dev.alloc_matrix(37, n, tdt, "cuda")
    w[:37, :n] = torch.as_tensor(ks, dtype=tdt)
    dev.trsm_rows(kbuf, n, ws, w, 37)
    dev.trsm_rows_lt(kbuf, n, ws, w, 37)
    want = np.linalg.solve(K, ks.T).T
    assert rel(w[:37, :n].double().cpu().numpy(), want) < (1e-11 if dt == "f64" else 1e-3)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_trsm_rows_lt_batched_equals_single(dev, dt):
    tdt = TDT[dt]
    n, m, nb = 1000, 37, 3
    ld = dev.padded_ld(n)
    wsb = (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16
    larena = torch.empty((nb, n, ld), dtype=tdt, device="cuda")
    wsarena = torch.empty((nb, wsb), dtype=torch.uint8, device="cuda")
    barena = torch.empty((nb, m, ld), dtype=tdt, device="cuda")
    singles = []
    rng = np.random.default_rng(5)
    for b in range(nb):
        _, _, kbuf, ws, _ = _factor(dev, n, tdt, seed=40 + b)
        larena[b].copy_(kbuf[:n])
        wsarena[b, :ws.numel()].copy_(ws)
        B = torch.as_tensor(rng.normal(size=(m, n)), dtype=tdt)
        barena[b, :, :n] = B
        one = dev.alloc_matrix(m, n, tdt, "cuda")
        one[:m, :n] = B
        dev.trsm_rows_lt(kbuf, n, ws, one, m)
        singles.append(one[:m, :n].clone())
    dev.trsm_rows_lt_batched(larena, n, wsarena, barena, m)
    for b in range(nb):
        assert torch.equal(barena[b, :, :n], singles[b])


# ---- the contraction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("q", [1, 3, 4, 5, 8])
def test_cov_predict_grad_matches_numpy(dev, cov, d, q):
    rng = np.random.default_rng(100 * cov + 10 * d + q)
    n, ns, ell, sf2 = 300, 45, 0.7, 1.3
    x = rng.uniform(-1, 1, size=(n, d))
    xs = rng.uniform(-1, 1, size=(ns, d))
    xs[0] = x[5]                                         # a test point on a training point (r = 0)
    alpha = rng.normal(size=(n, q))
    beta = rng.normal(size=(ns, n))
    want_m, want_v = contract(x, alpha, xs, cov, ell, sf2, beta)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    bbuf = dev.alloc_matrix(ns, n, torch.float64, "cuda")
    bbuf[:ns, :n] = T(beta)
    for mode in ("mean", "var", "both"):
        mg = torch.zeros((ns, d, q), dtype=torch.float64, device="cuda") if mode != "var" else None
        vg = torch.zeros((ns, d), dtype=torch.float64, device="cuda") if mode != "mean" else None
        dev.cov_predict_grad(T(x), T(alpha), T(xs), ell, sf2, beta=bbuf if vg is not None else None, mean_grad=mg, var_grad=vg,
                             cov=cov)
        if mg is not None:
            got = mg.cpu().numpy()
            assert np.isfinite(got).all() and rel(got, want_m) < 1e-12
        if vg is not None:
            got = vg.cpu().numpy()
            assert np.isfinite(got).all() and rel(got, want_v) < 1e-12
    # accumulate = 1 adds onto prefilled outputs
    pre_m, pre_v = rng.normal(size=(ns, d, q)), rng.normal(size=(ns, d))
    mg, vg = T(pre_m), T(pre_v)
    dev.cov_predict_grad(T(x), T(alpha), T(xs), ell, sf2, beta=bbuf, mean_grad=mg, var_grad=vg, accumulate=True, cov=cov)
    assert rel(mg.cpu().numpy(), pre_m + want_m) < 1e-12 and rel(vg.cpu().numpy(), pre_v + want_v) < 1e-12
    # f32
    T32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")
    b32 = dev.alloc_matrix(ns, n, torch.float32, "cuda")
    b32[:ns, :n] = T32(beta)
    mg32 = torch.zeros((ns, d, q), dtype=torch.float32, device="cuda")
    vg32 = torch.zeros((ns, d), dtype=torch.float32, device="cuda")
    dev.cov_predict_grad(T32(x), T32(alpha), T32(xs), ell, sf2, beta=b32, mean_grad=mg32, var_grad=vg32, cov=cov)
    assert rel(mg32.double().cpu().numpy(), want_m) < 1e-4 and rel(vg32.double().cpu().numpy(), want_v) < 1e-4


def test_matern12_at_a_training_point_follows_the_r0_convention(dev):
    x = np.array([[0.0], [0.5], [1.0]])
    alpha = np.ones((3, 1))
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")
    mg = torch.zeros((1, 1, 1), dtype=torch.float64, device="cuda")
    dev.cov_predict_grad(T(x), T(alpha), T(x[:1].copy()), 1.0, 1.0, mean_grad=mg, cov=1)
    want = -(np.exp(-0.5) / 0.5 * (0.0 - 0.5) + np.exp(-1.0) / 1.0 * (0.0 - 1.0))
    assert np.isfinite(mg.item()) and abs(mg.item() - want) < 1e-14


# ---- the model ------------------------------------------------------------------------------------------------------
def _kernels(ca, which):
    if which == "rbf":
        return [ca.RBFKernel(l=1.0 / 2 ** j, sf=1.0) for j in range(3)]
    return [ca.RBFKernel(l=1.0, sf=1.0), ca.DenseMaternKernel(nu=1.5, l=0.5, sf=0.8), ca.DenseMaternKernel(nu=2.5, l=0.3, sf=0.6)]


def _numpy_model_grad(m, xs_raw, iset):
    """The gradients built in NumPy from the fitted blocks' x, alpha and L (normalised units, then the chain rule)."""
    xs = np.asarray(xs_raw, dtype=np.float64)
    if m.standard_normalized_inputs:
        xs = (xs - m.mean_x_train) / m.std_x_train
    ns, d = xs.shape
    dm, dv = np.zeros((ns, d, m.dy)), np.zeros((ns, d))
    for j in range(iset.get_n_resolutions() + 1):
        k = m.posterior_obj[j].kernel
        for l, (a, b) in enumerate(iset.bounds[j]):
            a, b = int(a), int(b)
            if b <= a:
                continue
            blk = m.posterior_obj[j].blocks[l]
            x = blk.x.double().cpu().numpy()
            alpha = blk.alpha.double().cpu().numpy()
            L = np.tril(blk.lbuf[:blk.n, :blk.n].double().cpu().numpy())
            t = xs[a:b]
            ks = kcov(t, x, k.cov, k.l, k.sf)
            beta = sla.cho_solve((L, True), ks.T).T
            mg, vg = contract(x, alpha, t, k.cov, k.l, k.sf, beta)
            dm[a:b] += mg
            dv[a:b] += vg
    if m.standard_normalized_inputs:
        dm = dm / m.std_x_train[None, :, None]
        dv = dv / m.std_x_train[None, :]
    return dm, dv


def _problem(d, n, seed):
    from cimrgp_amd.Inputs import space_filling_order
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d)) * np.array([1.0, 3.0, 0.5][:d])
    x = x[space_filling_order(x)]
    y = np.stack([np.sin(2 * x[:, 0]) + 0.2 * x[:, -1], np.cos(1.5 * x[:, -1])], axis=1) + 0.05 * rng.normal(size=(n, 2))
    return x, y


@pytest.mark.parametrize("which", ["rbf", "mixed"])
@pytest.mark.parametrize("d,n", [(1, 600), (1, 601), (2, 1024)])
@pytest.mark.parametrize("normalized", [True, False])
def test_model_predictive_gradients(which, d, n, normalized):
    """n = 600: equal blocks, the batched path; n = 601: unequal blocks, the per-block path; d = 2: Hilbert order."""
    import cimrgp_amd as ca
    from cimrgp_amd.Inputs import space_filling_order
    x, y = _problem(d, n, seed=n + d)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, 2, 2), spectral_density_obj=_kernels(ca, which),
                                          standard_normalized_inputs=normalized)
    m.fit()
    if n == 600:
        assert any(len(bt.regions) >= 2 for p in m.posterior_obj for bt in p.batches)
    rng = np.random.default_rng(7)
    xs = rng.uniform(-1.8, 1.8, size=(130, d)) * np.array([1.0, 3.0, 0.5][:d])
    xs = xs[space_filling_order(xs)]
    iset = ca.IndexSetUniform(130, 2, 2)
    dmu, dvar = m.predictive_gradients(xs, iset)
    assert dmu.shape == (130, d, 2) and dvar.shape == (130, d)
    scale = np.abs(xs).max()
    fm, fv = central_diff(lambda t: m.get_predicted_mean_and_var(t, iset), xs, 1e-5 * scale)
    # a Matern 3/2 covariance has a kink in its second derivative at r = 0: central differences of the mixed chain
    # carry an O(h) error wherever a test point lies within h of a training point
    tol = 1e-6 if which == "rbf" else 2e-5
    assert rel(dmu, fm) < tol, rel(dmu, fm)
    assert rel(dvar, fv) < tol, rel(dvar, fv)
    wm, wv = _numpy_model_grad(m, xs, iset)
    assert rel(dmu, wm) < 1e-10 and rel(dvar, wv) < 1e-10


def test_model_root_only_and_errors():
    import cimrgp_amd as ca
    x, y = _problem(1, 300, seed=2)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(300, 1, 2), spectral_density_obj=_kernels(ca, "rbf")[:2])
    m.fit()
    xs = np.linspace(-1.5, 1.5, 40)[:, None]
    dmu, dvar = m.predictive_gradients(xs)                 # no index set: the root block serves every point
    fm, fv = central_diff(lambda t: m.get_predicted_mean_and_var(t), xs, 1e-5)
    assert rel(dmu, fm) < 1e-6 and rel(dvar, fv) < 1e-6
    m2 = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(300, 1, 2, first_divider_power=1),
                                           spectral_density_obj=_kernels(ca, "rbf")[:2])
    m2.fit()
    with pytest.raises(ValueError) as ref:
        m2.get_predicted_mean(xs)
    with pytest.raises(ValueError) as got:
        m2.predictive_gradients(xs)
    assert str(got.value) == str(ref.value)


# ---- the plugin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "ard", "matern"])
def test_plugin_predictive_gradients(kind):
    import cimrgp_amd as ca
    rng = np.random.default_rng(4)
    x = rng.uniform(-2, 2, size=(300, 2)) * np.array([1.0, 2.5])
    y = np.stack([np.sin(2 * x[:, 0]) + x[:, 1], np.cos(x[:, 1])], axis=1) + 0.1 * rng.normal(size=(300, 2))
    xs = rng.uniform(-2, 2, size=(50, 2))
    gp = {"rbf": lambda: ca.GP_RBF(optimize=False), "ard": lambda: ca.GP_RBF(ARD=True, lengthscale=0.7, optimize=False),
          "matern": lambda: ca.GP_Matern(2.5, optimize=False)}[kind]()
    if kind == "ard":
        gp = ca.GP_RBF(ARD=True, max_iters=30)              # learned per-dimension length-scales
    gp.fit((x, y))
    dmu, dvar = gp.predictive_gradients(xs)
    assert dmu.shape == (50, 2, 2) and dvar.shape == (50, 2)
    fm, fv = central_diff(lambda t: gp.predict_with_variance(t), xs, 1e-5)
    fm2, _ = central_diff(lambda t: (gp.predict(t), np.zeros(t.shape[0])), xs, 1e-5)
    assert rel(dmu, fm) < 1e-6 and rel(dmu, fm2) < 1e-6 and rel(dvar, fv) < 1e-6


# ---- buffer footprint -----------------------------------------------------------------------------------------------
def _lib():
    from cimrgp_amd import _lib as L
    return L


def _sync():
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m", [(300, 37), (513, 70)])
def test_trsm_rows_lt_footprint(dev, dt, n, m):
    tdt = TDT[dt]
    L_ = _lib()
    dtype = L_.F64 if dt == "f64" else L_.F32
    _, _, kbuf, ws, Lh = _factor(dev, n, tdt, seed=n)
    ld = wide_ld(n)
    lb = Guarded("L", (n + 3) * ld, tdt, "cuda", ld=ld)
    lb.mark(CONST, n, n, part="lower", values=torch.tril(kbuf[:n, :n]))
    esz = torch.empty((), dtype=tdt).element_size()
    wsb = Guarded("workspace", ws.numel() // esz, tdt, "cuda").vec(CONST, ws.numel() // esz, values=ws.view(tdt))
    B = np.random.default_rng(1).normal(size=(m, n))
    bb = Guarded("B", (m + 3) * ld, tdt, "cuda", ld=ld).mark(INOUT, m, n, values=B)
    lib = L_.load()

    def call():
        L_.check(lib.cimrgp_trsm_rows_lt(dtype, lb.ptr(), n, ld, wsb.ptr(), bb.ptr(), m, ld, torch.cuda.current_stream().cuda_stream),
                 "cimrgp_trsm_rows_lt")
    run_contract([lb, wsb, bb], call, _sync)
    want = sla.solve_triangular(Lh, B.T, trans="T", lower=True).T
    assert rel(bb.mat(m, n).double().cpu().numpy(), want) < (1e-11 if dt == "f64" else 2e-4)


@pytest.mark.parametrize("cov", [0, 1])
def test_layer_predict_grad_footprint(dev, cov):
    """Two blocks of a layer: the shared outputs are written at their test rows only (INOUT, accumulate), the W arena is
    a work area whose gaps and padding stay untouched."""
    L_ = _lib()
    tdt, n, ns, nb, d, q = torch.float64, 200, 24, 2, 2, 3
    rng = np.random.default_rng(3)
    N, Ns = nb * n + 17, nb * ns + 11
    x = rng.uniform(-1, 1, size=(N, d))
    xs = rng.uniform(-1, 1, size=(Ns, d))
    starts, t_starts = [5, 5 + n], [3, 3 + ns + 2]
    ld = wide_ld(n)
    lstride = (n + 2) * ld
    wsn = (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16 // 8
    la = Guarded("L", nb * lstride, tdt, "cuda", ld=ld)
    wa = Guarded("workspace", nb * wsn, tdt, "cuda")
    alphas, facs = [], []
    for b in range(nb):
        xb = x[starts[b]:starts[b] + n]
        K = kcov(xb, xb, cov, 0.6, 1.2) + 0.1 * np.eye(n)
        kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
        kbuf[:n, :n] = torch.as_tensor(K, dtype=tdt)
        ws, info = dev.potrf(kbuf, n)
        la.mark(CONST, n, n, off=b * lstride, part="lower", values=torch.tril(kbuf[:n, :n]))
        wa.vec(CONST, ws.numel() // 8, off=b * wsn, values=ws.view(tdt))
        alphas.append(rng.normal(size=(n, q)))
        facs.append((xb, K))
    xg = Guarded("x", N * d, tdt, "cuda").vec(CONST, N * d, values=x.reshape(-1))
    xsg = Guarded("xs", Ns * d, tdt, "cuda").vec(CONST, Ns * d, values=xs.reshape(-1))
    al = Guarded("alpha", nb * n * q, tdt, "cuda").vec(CONST, nb * n * q, values=np.concatenate(alphas).reshape(-1))
    st = Guarded("starts", nb, torch.int64, "cuda").vec(CONST, nb, values=np.array(starts))
    ts = Guarded("t_starts", nb, torch.int64, "cuda").vec(CONST, nb, values=np.array(t_starts))
    ldw = wide_ld(n)
    wstride = (ns + 1) * ldw
    w = Guarded("W", nb * wstride, tdt, "cuda", ld=ldw)
    for b in range(nb):
        w.mark(JUNK, ns, n, off=b * wstride)
    pre_m, pre_v = rng.normal(size=(Ns, d, q)), rng.normal(size=(Ns, d))
    mg = Guarded("mean_grad", Ns * d * q, tdt, "cuda")
    vg = Guarded("var_grad", Ns * d, tdt, "cuda")
    for b in range(nb):
        a = t_starts[b]
        mg.vec(INOUT, ns * d * q, off=a * d * q, values=pre_m[a:a + ns].reshape(-1))
        vg.vec(INOUT, ns * d, off=a * d, values=pre_v[a:a + ns].reshape(-1))
    lib = L_.load()

    def call():
        L_.check(lib.cimrgp_layer_predict_grad_cov(L_.F64, cov, xg.ptr(), st.ptr(), n, d, xsg.ptr(), ts.ptr(), ns, nb, 0.6, 1.2,
                                                   la.ptr(), ld, lstride, wa.ptr(), wsn * 8, al.ptr(), q, w.ptr(), ldw, wstride,
                                                   mg.ptr(), vg.ptr(), 1, torch.cuda.current_stream().cuda_stream),
                 "cimrgp_layer_predict_grad_cov")
    run_contract([la, wa, xg, xsg, al, st, ts, w, mg, vg], call, _sync)
    got_m = mg.data.view(Ns, d, q).cpu().numpy()
    got_v = vg.data.view(Ns, d).cpu().numpy()
    for b in range(nb):
        xb, K = facs[b]
        a = t_starts[b]
        t = xs[a:a + ns]
        beta = np.linalg.solve(K, kcov(t, xb, cov, 0.6, 1.2).T).T
        wm, wv = contract(xb, alphas[b], t, cov, 0.6, 1.2, beta)
        assert rel(got_m[a:a + ns], pre_m[a:a + ns] + wm) < 1e-10
        assert rel(got_v[a:a + ns], pre_v[a:a + ns] + wv) < 1e-10


def test_layer_predict_grad_mean_alone_matches_numpy(dev):
    """The batched call with mean_grad alone: no W is formed, d mean / d xs accumulates at each block's test rows and the
    rows between the blocks stay as they were."""
    tdt, nb, n, ns, d, q, cov, ell, sf2 = torch.float64, 2, 65, 33, 1, 3, 2, 0.6, 1.2
    rng = np.random.default_rng(11)
    N, Ns = nb * n + 17, nb * ns + 11
    x = rng.uniform(-1, 1, size=(N, d))
    xs = rng.uniform(-1, 1, size=(Ns, d))
    starts, t_starts = np.array([5, 5 + n]), np.array([3, 3 + ns + 2])
    alpha = rng.normal(size=(nb, n, q))
    pre = rng.normal(size=(Ns, d, q))
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda")
    larena = torch.zeros((nb, n, dev.padded_ld(n)), dtype=tdt, device="cuda")        # not read without var_grad
    ws_arena = torch.zeros((nb, (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    mg = T(pre)
    dev.layer_predict_grad(T(x), torch.as_tensor(starts).cuda(), n, T(xs), torch.as_tensor(t_starts).cuda(), ns, ell, sf2, larena,
                           ws_arena, T(alpha), mg, None, cov=cov)
    torch.cuda.synchronize()
    got = mg.cpu().numpy()
    seen = np.zeros(Ns, dtype=bool)
    for b in range(nb):
        a = t_starts[b]
        wm, _ = contract(x[starts[b]:starts[b] + n], alpha[b], xs[a:a + ns], cov, ell, sf2)
        assert rel(got[a:a + ns], pre[a:a + ns] + wm) < 1e-10
        seen[a:a + ns] = True
    assert np.array_equal(got[~seen], pre[~seen])
