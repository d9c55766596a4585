"""The joint predictive distribution on the GPU (include/cimrgp_joint.h, DESIGN.md "Joint predictive covariance and
posterior samples"): the normal generator against its NumPy restatement, the block covariance and its factor against
NumPy, the sampler against tril(L) Z, and the model / plugin methods against covariances built in NumPy from the
fitted blocks."""
import numpy as np
import pytest

from tests.test_joint_host import phi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NU = {1: 0.5, 2: 1.5, 3: 2.5}


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _kcov(xa, xb, cov, ell, sf2):
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    if cov == 0:
        return sf2 * np.exp(-d2 / (2 * ell * ell))
    nu = NU[cov]
    t = np.sqrt(2 * nu) * np.sqrt(d2) / ell
    poly = {0.5: 1.0, 1.5: 1 + t, 2.5: 1 + t + t * t / 3}[nu]
    return sf2 * poly * np.exp(-t)


def _keys(vals):
    return torch.tensor(vals, dtype=torch.int64).cuda()


# ---- cimrgp_normal_fill ---------------------------------------------------------------------------------------------
def test_normal_fill_matches_numpy_phi(dev):
    seed, keys = 0x1234567890ABCDEF, [(2 << 32) + 5, 0, (7 << 32) + 123]
    cols, ns = 9, 301
    ldz = dev.padded_ld(ns)
    z64 = torch.full((3, cols, ldz), 7.0, dtype=torch.float64, device="cuda")
    z32 = torch.full((3, cols, ldz), 7.0, dtype=torch.float32, device="cuda")
    dev.normal_fill(seed, _keys(keys), 0, cols, ns, z64)
    dev.normal_fill(seed, _keys(keys), 0, cols, ns, z32)
    g64, g32 = z64.cpu().numpy(), z32.cpu().numpy()
    for b, k in enumerate(keys):
        want = phi(seed, k, cols, ns)
        np.testing.assert_allclose(g64[b, :, :ns], want, rtol=0, atol=1e-14 * (1 + np.abs(want)).max())
        assert np.all(np.abs(g64[b, :, :ns] - want) <= 8 * np.spacing(np.abs(want)) + 1e-300 + 4e-16 * np.abs(want).max())
        np.testing.assert_array_equal(g32[b, :, :ns], g64[b, :, :ns].astype(np.float32))
        assert np.all(g64[b, :, ns:] == 7.0)           # nothing beyond ns
    # the same key in another batch, another column count and another column window: bit-identical values
    z1 = torch.zeros((1, 4, ldz), dtype=torch.float64, device="cuda")
    dev.normal_fill(seed, _keys([keys[2]]), 3, 4, ns, z1)
    np.testing.assert_array_equal(z1.cpu().numpy()[0, :, :ns], g64[2, 3:7, :ns])
    z2 = torch.zeros((1, 2, dev.padded_ld(100)), dtype=torch.float64, device="cuda")
    dev.normal_fill(seed, _keys([keys[2]]), 0, 2, 100, z2)
    np.testing.assert_array_equal(z2.cpu().numpy()[0, :, :100], g64[2, :2, :100])


def test_normal_fill_moments(dev):
    z = torch.empty((1, 1000, 1008), dtype=torch.float64, device="cuda")
    dev.normal_fill(2026, _keys([9]), 0, 1000, 1000, z)
    v = z[0, :, :1000].reshape(-1).cpu().numpy()
    se = 1.0 / np.sqrt(v.size)
    assert abs(v.mean()) < 5 * se
    assert abs(v.var() - 1.0) < 5 * np.sqrt(2.0) * se
    assert abs((v ** 3).mean()) < 5 * np.sqrt(15.0) * se
    assert abs((v ** 4).mean() - 3.0) < 5 * np.sqrt(96.0) * se


# ---- cimrgp_layer_joint_cov -----------------------------------------------------------------------------------------
def _fitted_layer(dev, nb, n, d, ns, cov, tdt, seed, ell=0.7, sf2=1.3):
    """A layer of nb blocks of n training points fitted by cimrgp_layer_fit_cov, and nb x ns test points."""
    rng = np.random.default_rng(seed)
    total = nb * n + 21
    x = rng.uniform(-1.5, 1.5, size=(total, d))
    x = x[np.argsort(x[:, 0])]
    y = np.stack([np.sin(2 * x[:, 0] + c) for c in range(2)], axis=1) + 0.1 * rng.normal(size=(total, 2))
    starts = np.array([5 + i * n for i in range(nb)], dtype=np.int64)
    xs = np.concatenate([x[s:s + n][rng.integers(0, n, size=ns)] + 0.05 * rng.normal(size=(ns, d)) for s in starts])
    t_starts = np.arange(nb, dtype=np.int64) * ns
    X, Y = dev.to_device(x, tdt, "cuda"), dev.to_device(y, tdt, "cuda")
    ld = dev.padded_ld(n)
    karena = torch.empty((nb, n, ld), dtype=tdt, device="cuda")
    wsb = max((dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16, 16)
    ws = torch.empty((nb, wsb), dtype=torch.uint8, device="cuda")
    info = torch.zeros(nb, dtype=torch.int32, device="cuda")
    bias = torch.empty((nb, 2), dtype=tdt, device="cuda")
    noise = torch.empty(nb, dtype=tdt, device="cuda")
    z = torch.empty((nb, n, 2), dtype=tdt, device="cuda")
    alpha = torch.empty((nb, n, 2), dtype=tdt, device="cuda")
    dev.layer_fit(X, Y, None, torch.zeros_like(Y), _keys(starts), n, ell, sf2, 0.05, 0.01, 1e-8, None, None, karena, ws, info,
                  bias, noise, z, alpha, cov=cov)
    assert int(info.abs().max()) == 0
    return dict(x=x, X=X, starts=starts, xs=xs, XS=dev.to_device(xs, tdt, "cuda"), t_starts=t_starts, karena=karena, ws=ws,
                n=n, ns=ns, nb=nb, ell=ell, sf2=sf2, cov=cov, noise=0.05)


def _sigma(L, b, diag):
    x = L["x"][L["starts"][b]:L["starts"][b] + L["n"]]
    xs = L["xs"][L["t_starts"][b]:L["t_starts"][b] + L["ns"]]
    k = _kcov(x, x, L["cov"], L["ell"], L["sf2"]) + L["noise"] * np.eye(L["n"])
    ks = _kcov(xs, x, L["cov"], L["ell"], L["sf2"])
    return _kcov(xs, xs, L["cov"], L["ell"], L["sf2"]) - ks @ np.linalg.solve(k, ks.T) + diag * np.eye(L["ns"])


def _joint(dev, L, diag, factor, tdt):
    nb, ns = L["nb"], L["ns"]
    ldc = dev.padded_ld(ns)
    c = torch.full((nb, ns, ldc), 5.0, dtype=tdt, device="cuda")
    cws = info = None
    if factor:
        cws = torch.empty((nb, max((dev.potrf_workspace_bytes(ns, tdt) + 15) // 16 * 16, 16)), dtype=torch.uint8, device="cuda")
        info = torch.full((nb,), -9, dtype=torch.int32, device="cuda")
    dev.layer_joint_cov(L["X"], _keys(L["starts"]), L["n"], L["XS"], _keys(L["t_starts"]), ns, L["ell"], L["sf2"], L["karena"],
                        L["ws"], torch.tensor(diag, dtype=tdt, device="cuda"), c, cws, info, cov=L["cov"])
    return c, info


@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("tdt", [torch.float64, torch.float32])
@pytest.mark.parametrize("nb,n,ns", [(1, 64, 1), (3, 700, 17), (16, 64, 256), (3, 2048, 256), (1, 4100, 1500)])
def test_layer_joint_cov_matches_numpy(dev, cov, tdt, nb, n, ns):
    L = _fitted_layer(dev, nb, n, 2, ns, cov, tdt, seed=nb * 1000 + n + cov)
    diag = [0.01 * (b + 1) for b in range(nb)]
    c, _ = _joint(dev, L, diag, False, tdt)
    cf, info = _joint(dev, L, diag, True, tdt)
    eps = np.finfo(np.float32 if tdt == torch.float32 else np.float64).eps
    for b in range(nb):
        want = _sigma(L, b, diag[b])
        got = np.tril(c[b, :, :ns].double().cpu().numpy())
        err = np.max(np.abs(got - np.tril(want))) / np.max(np.abs(want))
        assert err < ((5e-2 if n > 2048 else 1e-2) if tdt == torch.float32 else 1e-9), (b, err)
        lf = cf[b, :, :ns].double().cpu().numpy()
        assert np.all(np.triu(lf, 1) == 0.0)
        assert np.all(cf[b, :, ns:].cpu().numpy() == 5.0)         # padding is the caller's
        cd = np.tril(got) + np.tril(got, -1).T
        berr = np.linalg.norm(lf @ lf.T - cd) / np.linalg.norm(cd)
        assert berr < 8 * ns * eps + 1e-14, (b, berr)
    assert int(info.abs().max()) == 0


def test_layer_joint_cov_failure_isolation(dev):
    tdt = torch.float64
    L = _fitted_layer(dev, 3, 128, 1, 40, 0, tdt, seed=3, ell=0.05)
    # block 1: identical test points far from every training point -> Sigma = sf2 J, second pivot exactly 0
    xs = L["xs"].copy()
    xs[40:80] = 1e3
    L["xs"], L["XS"] = xs, dev.to_device(xs, tdt, "cuda")
    c0, info = _joint(dev, L, [1e-3, 0.0, 1e-3], True, tdt)
    info = info.cpu().numpy()
    assert list(info) == [0, 2, 0]
    for b in (0, 2):
        want = np.linalg.cholesky(_sigma(L, b, 1e-3))
        got = c0[b, :, :40].cpu().numpy()
        assert np.max(np.abs(got - want)) < 1e-8


# ---- cimrgp_layer_sample --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [torch.float64, torch.float32])
@pytest.mark.parametrize("nb,ns,cols", [(1, 1, 1), (3, 17, 5), (2, 300, 40), (4, 256, 512), (1, 1500, 130)])
def test_layer_sample_matches_numpy(dev, tdt, nb, ns, cols):
    rng = np.random.default_rng(ns + cols)
    ldl = dev.joint_ld(ns, tdt) + 16
    lar = torch.tensor(rng.normal(size=(nb, ns, ldl)), dtype=tdt, device="cuda")
    ii = torch.arange(ns, device="cuda")
    lar[:, :, :ns].masked_fill_((ii[None, :] > ii[:, None])[None], float("nan"))     # strict upper: NaN, never read
    lar[:, :, ns:] = float("nan")
    ldz = dev.joint_ld(ns, tdt)
    z = torch.empty((nb, cols, ldz), dtype=tdt, device="cuda")
    dev.normal_fill(11, _keys(list(range(nb))), 0, cols, ns, z)
    z[:, :, ns:] = float("nan")
    gap = 7
    t_starts = np.array([3 + b * (ns + gap) for b in range(nb)], dtype=np.int64)
    ld_out = int(t_starts[-1]) + ns + 5
    prior = rng.normal(size=(cols, ld_out))
    out = torch.tensor(prior, dtype=tdt, device="cuda")
    dev.layer_sample(lar, ns, z, cols, _keys(t_starts), out)
    dev.layer_sample(lar, ns, z, cols, _keys(t_starts), out)        # accumulates
    got = out.double().cpu().numpy()
    want = prior.copy()
    Lh = np.tril(np.nan_to_num(lar.double().cpu().numpy(), nan=0.0)[:, :, :ns])
    Zh = z.double().cpu().numpy()[:, :, :ns]
    for b in range(nb):
        a = t_starts[b]
        want[:, a:a + ns] += 2 * (Zh[b] @ Lh[b].T)
    tol = (1e-4 if tdt == torch.float32 else 1e-12) * np.sqrt(ns) * 4
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - want)) < tol * max(1.0, np.abs(want).max())
    # untouched outside the blocks' ranges
    mask = np.ones(ld_out, dtype=bool)
    for a in t_starts:
        mask[a:a + ns] = False
    np.testing.assert_array_equal(got[:, mask], prior[:, mask].astype(np.float32 if tdt == torch.float32 else np.float64))


# ---- the model ------------------------------------------------------------------------------------------------------
def _model(ca, kernels, n=600, d=1, res=2, seed=5, dtype="f64", shared=False, **kw):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d))
    x = x[np.argsort(x[:, 0])]
    y = np.stack([np.sin(3 * x[:, 0]) + 0.3 * x[:, -1], np.cos(2 * x[:, 0])], axis=1) + 0.1 * rng.normal(size=(n, 2))
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2), spectral_density_obj=kernels,
                                          dtype=dtype, bias_region_specific=not shared, noise_region_specific=not shared, **kw)
    m.fit()
    return m, x, y


class _OracleGram(object):
    """oracle.dense.rbf_gram replaced, for the duration of a with block, by the covariance of the layer whose
    length-scale it is called with (the oracle's chain builds every Gram through it; tests/test_gpu_matern.py does
    the same): the oracle fits layers of any covariance."""

    def __init__(self, kernels):
        self.by_ell = {float(k.l): k for k in kernels}
        assert len(self.by_ell) == len(kernels), "the layers' length-scales must differ"

    def __enter__(self):
        import oracle.dense as odense
        self.odense, self.saved = odense, odense.rbf_gram

        def gram(xa, xb=None, ell=1.0, sf2=1.0, diag_add=0.0):
            k = self.by_ell[float(ell)]
            out = _kcov(xa, xa if xb is None else xb, k.cov, ell, sf2)
            return out + diag_add * np.eye(xa.shape[0]) if xb is None else out
        odense.rbf_gram = gram
        return self

    def __exit__(self, *exc):
        self.odense.rbf_gram = self.saved


def _oracle_sigma(kernels, x, y, shared, xs_raw, index_set, include_noise, jitter=None):
    """Per layer and region Sigma_jl (+ noise, + jitter sf2) in NumPy from the ORACLE's fit of the same data
    (oracle.mrgp_fit: its own input normalisation, bias and noise rule), independent of the model under test."""
    import oracle
    res = len(kernels) - 1
    xn, _, mu, sd = oracle.normalize_inputs(x)
    specs = [oracle.DenseLayerSpec(k.l, k.sf, k.noise) for k in kernels]
    with _OracleGram(kernels):
        omodel, _ = oracle.mrgp_fit(xn, y, oracle.index_bounds_uniform(x.shape[0], res, 2), specs, not shared, not shared)
    xs = (np.asarray(xs_raw, dtype=np.float64) - mu) / sd
    n_layers = index_set.get_n_resolutions() + 1
    out = []
    for j in range(n_layers):
        k = kernels[j]
        for l, (a, b) in enumerate(index_set.bounds[j]):
            a, b = int(a), int(b)
            blk = omodel[j][l]
            xb, t = xn[blk["a"]:blk["b"]], xs[a:b]
            kx = _kcov(xb, xb, k.cov, k.l, k.sf) + blk["noise"] * np.eye(xb.shape[0])
            ks = _kcov(t, xb, k.cov, k.l, k.sf)
            sig = _kcov(t, t, k.cov, k.l, k.sf) - ks @ np.linalg.solve(kx, ks.T)
            if include_noise and j == n_layers - 1:
                sig = sig + blk["noise"] * np.eye(b - a)
            if jitter is not None:
                sig = sig + jitter * k.sf * np.eye(b - a)
            out.append((j, l, a, b, sig))
    return out


def _chain(ca, res=2):
    return [ca.RBFKernel(l=1.0 / 2 ** j, sf=1.0) for j in range(res + 1)]


def _mixed(ca):
    return [ca.RBFKernel(l=1.0, sf=1.0), ca.DenseMaternKernel(nu=1.5, l=0.5, sf=0.8), ca.DenseMaternKernel(nu=2.5, l=0.3, sf=0.6)]


@pytest.mark.parametrize("which,d,shared", [("chain", 1, False), ("mixed", 2, True)])
@pytest.mark.parametrize("include_noise", [True, False])
def test_model_covariance(which, d, shared, include_noise):
    import cimrgp_amd as ca
    kernels = _chain(ca) if which == "chain" else _mixed(ca)
    m, x, y = _model(ca, kernels, d=d, shared=shared)
    rng = np.random.default_rng(1)
    xs = np.sort(rng.uniform(-2, 2, size=(150, d)), axis=0)
    iset = ca.IndexSetUniform(150, 2, 2)
    cov = m.get_predicted_covariance(xs, iset, include_noise=include_noise)
    assert cov.shape == (150, 150) and np.array_equal(cov, cov.T)
    _, var = m.get_predicted_mean_and_var(xs, iset, include_noise=include_noise)
    np.testing.assert_allclose(np.diag(cov), var, rtol=1e-12, atol=1e-12 * np.abs(var).max())
    want = np.zeros((150, 150))
    blocks = _oracle_sigma(kernels, x, y, shared, xs, iset, include_noise)
    for j, l, a, b, s in blocks:
        want[a:b, a:b] += s
    assert np.max(np.abs(cov - want)) < 1e-9 * np.abs(want).max()
    # entries between different finest regions carry only the coarser layers' terms
    fine = iset.bounds[2]
    a0, b0 = (int(v) for v in fine[0])
    a1, b1 = (int(v) for v in fine[1])
    coarse = np.zeros((b0 - a0, b1 - a1))
    for j, l, a, b, s in blocks:
        if j < 2 and a <= a0 and b >= b1:
            coarse += s[a0 - a:b0 - a, a1 - a:b1 - a]
    assert np.max(np.abs(cov[a0:b0, a1:b1] - coarse)) < 1e-9 * np.abs(want).max()


def _exact_dev(kernels, x, y, xs, iset, include_noise, jitter, seed, size):
    dy = y.shape[1]
    ns = xs.shape[0]
    want = np.zeros((size * dy, ns))
    for j, l, a, b, s in _oracle_sigma(kernels, x, y, False, xs, iset, include_noise, jitter=jitter):
        z = phi(seed, (j << 32) + l, size * dy, b - a)
        want[:, a:b] += z @ np.linalg.cholesky(s).T
    return want.reshape(size, dy, ns).transpose(0, 2, 1)


@pytest.mark.parametrize("which,d", [("chain", 1), ("mixed", 2)])
def test_model_samples_exact_and_reproducible(which, d):
    import cimrgp_amd as ca
    kernels = _chain(ca) if which == "chain" else _mixed(ca)
    m, x, y = _model(ca, kernels, d=d)
    rng = np.random.default_rng(2)
    xs = np.sort(rng.uniform(-2, 2, size=(120, d)), axis=0)
    iset = ca.IndexSetUniform(120, 2, 2)
    mean = m.get_predicted_mean(xs, iset)
    s20 = m.posterior_samples(xs, 20, iset, seed=77, jitter=1e-3)
    assert s20.shape == (20, 120, 2)
    want = _exact_dev(kernels, x, y, xs, iset, True, 1e-3, 77, 20)
    assert np.max(np.abs((s20 - mean[None]) - want)) < 1e-9 * np.abs(want).max()
    assert m.last_joint_jitter == [1e-3] * 3
    np.testing.assert_array_equal(m.posterior_samples(xs, 20, iset, seed=77, jitter=1e-3), s20)
    np.testing.assert_array_equal(m.posterior_samples(xs, 5, iset, seed=77, jitter=1e-3), s20[:5])
    other = m.posterior_samples(xs, 20, iset, seed=78, jitter=1e-3)
    assert not np.any(other == s20)


def test_model_samples_monte_carlo():
    import cimrgp_amd as ca
    m, x, y = _model(ca, _chain(ca, 1), n=200, res=1)
    xs = np.linspace(-1.9, 1.9, 24)[:, None]
    iset = ca.IndexSetUniform(24, 1, 2)
    cov = m.get_predicted_covariance(xs, iset)
    s = m.posterior_samples(xs, 20000, iset, seed=3, jitter=0.0)
    mean = m.get_predicted_mean(xs, iset)
    for o in range(2):
        dlt = s[:, :, o] - mean[None, :, o]
        emp = dlt.T @ dlt / s.shape[0]
        se = np.sqrt((cov ** 2 + np.outer(np.diag(cov), np.diag(cov))) / s.shape[0])
        assert np.all(np.abs(emp - cov) < 5 * se + 1e-12)


def test_model_jitter_escalation_and_failure():
    import cimrgp_amd as ca
    m, x, y = _model(ca, _chain(ca, 1), n=200, res=1)
    # identical test points far from every training point: K* underflows to 0 and Sigma = sf2 J exactly, so a zero
    # jitter fails at the second pivot and the first escalation (1e-6) succeeds
    xs = np.full((32, 1), 1e3)
    iset = ca.IndexSetUniform(32, 1, 2)
    s = m.posterior_samples(xs, 4, iset, seed=1, include_noise=False, jitter=0.0)
    assert np.all(np.isfinite(s))
    assert m.last_joint_jitter == [1e-6, 1e-6]
    bad = np.linspace(-1.5, 1.5, 32)[:, None]
    bad[3] = np.nan                                        # hopeless: no jitter makes a NaN block positive definite
    with pytest.raises(np.linalg.LinAlgError, match="layer 0, region 0"):
        m.posterior_samples(bad, 4, iset, seed=1, jitter=1e-6)


def test_model_fp32_moments():
    import cimrgp_amd as ca
    m, x, y = _model(ca, _chain(ca, 1), n=300, res=1, dtype="f32")
    m64, _, _ = _model(ca, _chain(ca, 1), n=300, res=1)
    xs = np.linspace(-1.9, 1.9, 40)[:, None]
    iset = ca.IndexSetUniform(40, 1, 2)
    c32 = m.get_predicted_covariance(xs, iset)
    c64 = m64.get_predicted_covariance(xs, iset)
    # K** - W W^T cancels from sf2 = 1 down to ~1e-4: FP32 holds it to a small multiple of sf2 x 1e-5
    assert np.max(np.abs(c32 - c64)) < 1e-4
    s = m.posterior_samples(xs, 4000, iset, seed=5, jitter=1e-6)
    dlt = s - m.get_predicted_mean(xs, iset)[None]
    emp = np.einsum("sio,sjo->ij", dlt, dlt) / (2 * s.shape[0])
    want = c32 + sum(m.last_joint_jitter) * np.eye(40)           # sf2 = 1 in both layers
    assert np.max(np.abs(emp - want)) < 0.1 * np.abs(want).max()


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _two_rank_joint_worker(rank, world, port, out_dir):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    if world > 1:
        td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    rng = np.random.default_rng(21)
    n, ns, res = 640, 200, 3
    x = np.sort(rng.uniform(-2, 2, size=(n, 1)), axis=0)
    y = np.hstack([np.sin(3 * x), np.cos(5 * x) * x]) + 0.1 * rng.normal(size=(n, 2))
    xs = np.sort(rng.uniform(-2, 2, size=(ns, 1)), axis=0)
    kernels = [ca.RBFKernel(l=1.0 / 2 ** j, sf=1.0) for j in range(res + 1)]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2), spectral_density_obj=kernels)
    assert (model.rank, model.world_size) == (rank, world)
    model.fit()
    iset = ca.IndexSetUniform(ns, res, 2)
    cov = model.get_predicted_covariance(xs, iset)
    s = model.posterior_samples(xs, 6, iset, seed=9, jitter=1e-4)
    owned = [len(model._owned(j)) for j in range(res + 1)]
    np.savez(os.path.join(out_dir, "w%d_rank%d.npz" % (world, rank)), cov=cov, s=s, owned=np.array(owned))
    if world > 1:
        td.destroy_process_group()


def test_two_rank_joint_matches_one_rank(tmp_path):
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_two_rank_joint_worker, args=(0, 1, 0, str(tmp_path)))
    p.start()
    p.join(300)
    assert p.exitcode == 0
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = [ctx.Process(target=_two_rank_joint_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for q in procs:
        q.start()
    for q in procs:
        q.join(300)
    assert all(q.exitcode == 0 for q in procs), [q.exitcode for q in procs]
    one = np.load(tmp_path / "w1_rank0.npz")
    # ownership really was split: every block on exactly one of the two ranks, the finest layer shared out
    owned = [np.load(tmp_path / ("w2_rank%d.npz" % r))["owned"] for r in range(2)]
    np.testing.assert_array_equal(owned[0] + owned[1], one["owned"])
    assert owned[0][-1] > 0 and owned[1][-1] > 0
    for r in range(2):
        two = np.load(tmp_path / ("w2_rank%d.npz" % r))
        assert np.max(np.abs(two["cov"] - one["cov"])) < 1e-12 * np.abs(one["cov"]).max()
        assert np.max(np.abs(two["s"] - one["s"])) < 1e-10 * np.abs(one["s"]).max()


# ---- the plugin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern", "ard"])
def test_plugin_covariance_and_samples(kind):
    import cimrgp_amd as ca
    rng = np.random.default_rng(4)
    x = rng.uniform(-2, 2, size=(300, 2))
    y = np.stack([np.sin(2 * x[:, 0]) + x[:, 1], np.cos(x[:, 1])], axis=1) + 0.1 * rng.normal(size=(300, 2))
    xs = rng.uniform(-2, 2, size=(60, 2))
    gp = {"rbf": lambda: ca.GP_RBF(optimize=False), "matern": lambda: ca.GP_Matern(1.5, optimize=False),
          "ard": lambda: ca.GP_RBF(ARD=True, optimize=False)}[kind]()
    gp.fit((x, y))
    mean, cov = gp.predict_with_covariance(xs)
    m2, var = gp.predict_with_variance(xs)
    np.testing.assert_allclose(mean, m2, rtol=1e-10, atol=1e-12)     # (the mean-only and the mean-and-variance paths)
    np.testing.assert_allclose(np.diag(cov), var, rtol=1e-12, atol=1e-14)
    # against the oracle's fit of the plugin (oracle.gp_rbf_fit: its own z-scoring and noise rule, GPy's fixed l = 1,
    # sf2 = 1; ARD with optimize=False keeps unit length-scales, the isotropic covariance), covariance in NumPy
    import oracle
    k = ca.DenseMaternKernel(1.5, l=1.0, sf=1.0) if kind == "matern" else ca.RBFKernel(l=1.0, sf=1.0)
    with _OracleGram([k]):
        st = oracle.gp_rbf_fit(x, y)
    xz, noise, fit = st["xz"], st["noise"], st["fit"]
    t = oracle.zscore_apply(st["stats"], inputs=xs)
    kx = _kcov(xz, xz, k.cov, 1.0, 1.0) + noise * np.eye(300)
    ks = _kcov(t, xz, k.cov, 1.0, 1.0)
    want = _kcov(t, t, k.cov, 1.0, 1.0) - ks @ np.linalg.solve(kx, ks.T)
    assert np.max(np.abs(cov - want)) < 1e-9 * np.abs(want).max()
    zmean = ks @ fit["alpha"]
    assert np.max(np.abs(mean - oracle.zscore_apply(st["stats"], inverse_labels=zmean))) < 1e-8 * np.abs(mean).max()
    f = gp.posterior_samples_f(xs, size=3, seed=8)
    z = phi(8, 0, 6, 60)
    dz = (z @ np.linalg.cholesky(want + 1e-6 * np.eye(60)).T).reshape(3, 2, 60).transpose(0, 2, 1)
    fw = oracle.zscore_apply(st["stats"], inverse_labels=zmean[None] + dz)
    assert np.max(np.abs(f - fw)) < 1e-8 * np.abs(fw).max()
