"""GPU tests of the leave-one-out cross-validation (include/cimrgp_loo.h): the triangular inverse's row strips against
SciPy, diag(K^-1) against NumPy and bit for bit across strip heights, FP32 against the route through cimrgp_trsm_rows,
the model's and the plugin's methods against the NumPy restatement (tests/loo_numpy.py) and against refits on the device,
and one rank against two."""
import os
import socket

import numpy as np
import pytest

from loo_numpy import kcov, kinv_diag, loo_log_density, rel, trtri

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _factor(dev, n, tdt, seed, cov=0, d=2):
    """A device factor of K = k(x, x) + 1e-2 sf2 I with its strict upper triangle and padding poisoned: (lbuf, ws, L)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d))
    sf2 = 1.0
    ell = 0.8 if n <= 2048 else 0.25                # more points in the same box: a shorter scale keeps cond(K) ~ 1e4
    K = kcov(x, x, cov, ell, sf2) + 1e-2 * sf2 * np.eye(n)
    kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
    kbuf[:n, :n] = torch.as_tensor(K, dtype=tdt)
    ws, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    L = np.tril(kbuf[:n, :n].double().cpu().numpy())
    low = torch.tril(kbuf[:n, :n]).clone()
    kbuf.fill_(float("nan"))
    kbuf[:n, :n] = torch.where(torch.tril(torch.ones(n, n, dtype=torch.bool, device="cuda")), low, kbuf[:n, :n])
    return kbuf, ws, L


def _rowwise(got, want):
    """Largest row error relative to the row's norm in the reference."""
    return float(np.max(np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)))


# ---- rows of L^-T ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 700, 2048, 5632])
def test_trtri_rows_matches_scipy(dev, n):
    kbuf, ws, L = _factor(dev, n, torch.float64, seed=n)
    want = trtri(L)
    u = dev.alloc_matrix(n, n, torch.float64, "cuda")
    u.fill_(float("nan"))
    dev.trtri_rows(kbuf, n, ws, 0, n, out=u)
    whole = u[:n, :n].cpu().numpy()
    assert np.isfinite(whole).all()
    assert (np.tril(whole, -1) == 0).all()                      # zeros left of the diagonal are written
    assert torch.isnan(u[:n, n:]).all()                          # padding columns are not
    err = _rowwise(whole, want)
    print("trtri_rows n=%d row-wise relative error %.3e" % (n, err))
    assert err <= 1e-9
    # strips with r0 > 0 and a ragged m: the same bits, and nothing left of r0 is touched
    for r0, m in ((0, min(n, 100)), (256, n - 256), (256, 37), (512, 129), ((n - 1) // 256 * 256, n - (n - 1) // 256 * 256)):
        if r0 >= n or m <= 0 or r0 + m > n:
            continue
        s = dev.alloc_matrix(m, n, torch.float64, "cuda")
        s.fill_(float("nan"))
        dev.trtri_rows(kbuf, n, ws, r0, m, out=s)
        assert torch.isnan(s[:m, :r0]).all() and torch.isnan(s[:m, n:]).all()
        assert torch.equal(s[:m, r0:n].view(torch.int64), u[r0:r0 + m, r0:n].view(torch.int64)), (n, r0, m)


# ---- diag(K^-1) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 700, 2048, 5632])
def test_kinv_diag_matches_numpy_and_is_bit_equal_across_strips(dev, n):
    kbuf, ws, L = _factor(dev, n, torch.float64, seed=3 * n + 1, cov=2)
    want = kinv_diag(L)
    outs = []
    for strip in (256, 1024, n):
        outs.append(dev.kinv_diag(kbuf, n, ws, dev.kinv_diag_scratch_bytes(n, strip, torch.float64)))
    err = rel(outs[0].cpu().numpy() / want, np.ones(n))
    print("kinv_diag n=%d relative error %.3e" % (n, err))
    assert err <= 1e-9
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int64), outs[0].view(torch.int64))
    # and from cimrgp_trtri_rows on the whole matrix, reduced on the host in a fixed order
    u = dev.trtri_rows(kbuf, n, ws, 0, n)[:n, :n].cpu().numpy()
    assert rel((u ** 2).sum(axis=1) / want, np.ones(n)) <= 1e-9


@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("n", [300, 1100])
def test_kinv_diag_batched(dev, batch, n):
    tdt = torch.float64
    ld = dev.padded_ld(n) + 16
    wsb = (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16
    karena = torch.full((batch, n + 2, ld), float("nan"), dtype=tdt, device="cuda")
    ws_arena = torch.zeros((batch, wsb + 32), dtype=torch.uint8, device="cuda")
    Ls = []
    for b in range(batch):
        kbuf, ws, L = _factor(dev, n, tdt, seed=100 * batch + b, cov=b % 4)
        karena[b, :n, :n] = kbuf[:n, :n]
        ws_arena[b, :ws.numel()] = ws.view(torch.uint8)
        Ls.append(L)
    want = np.stack([kinv_diag(L) for L in Ls])
    outs = [dev.kinv_diag_batched(karena, n, ws_arena, batch * dev.kinv_diag_scratch_bytes(n, s, tdt)) for s in (256, 1024, n)]
    assert rel(outs[0].cpu().numpy() / want, np.ones_like(want)) <= 1e-9
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int64), outs[0].view(torch.int64))


@pytest.mark.parametrize("n", [700, 4096])
def test_kinv_diag_fp32_is_no_worse_than_the_route_through_trsm_rows(dev, n):
    """FP32 has no derived bar: the yardstick is the existing route to the same numbers (the identity through
    cimrgp_trsm_rows, rows squared and summed) on the same factor, both against the FP64 NumPy value.  Both errors are
    printed here; tools/bench_loo.py records them in profiles/loo_times.jsonl (case "kinv_diag_fp32_error")."""
    tdt = torch.float32
    kbuf, ws, L = _factor(dev, n, tdt, seed=n + 5)
    want = kinv_diag(L)
    new = dev.kinv_diag(kbuf, n, ws, dev.kinv_diag_scratch_bytes(n, 1024, tdt)).double().cpu().numpy()
    clean = torch.tril(torch.nan_to_num(kbuf[:n, :n], nan=0.0))
    kb2 = dev.alloc_matrix(n, n, tdt, "cuda")
    kb2.zero_()
    kb2[:n, :n] = clean
    eye = dev.alloc_matrix(n, n, tdt, "cuda")
    eye.zero_()
    eye[:n, :n].fill_diagonal_(1.0)
    dev.trsm_rows(kb2, n, ws, eye, n)
    old = (eye[:n, :n] ** 2).sum(dim=1).double().cpu().numpy()
    ea, eb = rel(new / want, np.ones(n)), rel(old / want, np.ones(n))
    print("kinv_diag FP32 n=%d: new %.3e, through trsm_rows %.3e (relative to FP64 NumPy)" % (n, ea, eb))
    assert np.isfinite(new).all()
    assert ea <= 2 * eb, (ea, eb)
    bit = dev.kinv_diag(kbuf, n, ws, dev.kinv_diag_scratch_bytes(n, n, tdt))
    assert torch.equal(bit.view(torch.int32), torch.as_tensor(new, dtype=tdt).cuda().view(torch.int32))


def test_loo_tail(dev):
    rng = np.random.default_rng(0)
    for tdt in (torch.float64, torch.float32):
        for q in (1, 3, 8):
            n = 777
            y, a, d = rng.normal(size=(n, q)), rng.normal(size=(n, q)), rng.uniform(0.5, 2, size=n)
            yt, at, dt_ = (torch.as_tensor(v, dtype=tdt).cuda() for v in (y, a, d))
            mean = torch.full((n, q), float("nan"), dtype=tdt, device="cuda")
            var = torch.full((n,), float("nan"), dtype=tdt, device="cuda")
            dev.loo(yt, at, dt_, mean, var)
            tol = 1e-14 if tdt == torch.float64 else 1e-6
            assert rel(mean.double().cpu().numpy(), y - a / d[:, None]) < tol and rel(var.double().cpu().numpy(), 1 / d) < tol
            dev.loo(yt, at, dt_, None, var)
            dev.loo(yt, at, dt_, mean, None)


# ---- the model ------------------------------------------------------------------------------------------------------
def _problem(d, n, seed):
    from cimrgp_amd.Inputs import space_filling_order
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d)) * np.array([1.0, 3.0, 0.5][:d])
    x = x[space_filling_order(x)]
    y = np.stack([np.sin(2 * x[:, 0]) + 0.2 * x[:, -1], np.cos(1.5 * x[:, -1])], axis=1) + 0.05 * rng.normal(size=(n, 2))
    return x, y


def _kernels(ca, which, noise=1e-2):
    nz = (lambda sf: None) if noise is None else (lambda sf: noise * sf)
    if which == "rbf":
        return [ca.RBFKernel(l=1.0 / 2 ** j, sf=1.0, noise=nz(1.0)) for j in range(3)]
    return [ca.RBFKernel(l=1.0, sf=1.0, noise=nz(1.0)), ca.DenseMaternKernel(nu=1.5, l=0.5, sf=0.8, noise=nz(0.8)),
            ca.DenseMaternKernel(nu=2.5, l=0.3, sf=0.6, noise=nz(0.6))]


def _numpy_model_loo(m, j):
    """The NumPy restatement from the fitted blocks of layer j: y - alpha / d and 1 / d, d from each block's factor."""
    y = m.observations
    mean, var = np.zeros_like(y), np.zeros(y.shape[0])
    for l, (a, b) in enumerate(m.index_set_obj.bounds[j]):
        a, b = int(a), int(b)
        blk = m.posterior_obj[j].blocks[l]
        L = np.tril(blk.lbuf[:blk.n, :blk.n].double().cpu().numpy())
        d = kinv_diag(L)
        mean[a:b] = y[a:b] - blk.alpha.double().cpu().numpy() / d[:, None]
        var[a:b] = 1.0 / d
    return mean, var


def _check_model(m, layers=(0, 1, 2)):
    y = m.observations
    for j in layers:
        mean, var = m.leave_one_out(j)
        wm, wv = _numpy_model_loo(m, j)
        assert mean.shape == y.shape and var.shape == (y.shape[0],)
        assert rel(mean, wm) <= 1e-9 and rel(var, wv) <= 1e-9, (j, rel(mean, wm), rel(var, wv))
        want = np.mean(-0.5 * np.log(2 * np.pi * wv) - 0.5 * (np.linalg.norm(y - wm, axis=1) ** 2) / wv)
        assert abs(m.get_loo_likelihood(j) - want) <= 1e-9 * abs(want)
    mean, var = m.leave_one_out()
    last, _ = m.leave_one_out(m.n_layers - 1)
    assert np.array_equal(mean, last)


@pytest.mark.parametrize("which", ["rbf", "mixed"])
@pytest.mark.parametrize("d,n", [(1, 600), (1, 601), (2, 1024)])
def test_model_leave_one_out(which, d, n):
    """n = 600 / 1024: equal regions, the batched path; n = 601: ragged regions, the per-block path as well."""
    import cimrgp_amd as ca
    x, y = _problem(d, n, seed=n + d)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, 2, 2), spectral_density_obj=_kernels(ca, which))
    m.fit()
    if n != 601:
        assert any(len(bt.regions) >= 2 for p in m.posterior_obj for bt in p.batches)
    _check_model(m)


@pytest.mark.parametrize("kw", [dict(optimize_hyperparameters=True, max_iters=15), dict(bias_region_specific=False),
                                dict(noise_region_specific=False), dict(bias_region_specific=False, noise_region_specific=False)])
def test_model_leave_one_out_learned_and_shared(kw):
    import cimrgp_amd as ca
    x, y = _problem(1, 600, seed=11)
    noise = None if "noise_region_specific" in kw else 1e-2
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(600, 2, 2),
                                          spectral_density_obj=_kernels(ca, "mixed", noise), **kw)
    m.fit()
    _check_model(m)


def test_model_leave_one_out_matches_refits_on_the_device(dev):
    """Eight points of one fitted block, each against a fresh DenseBlock fitted on the other n - 1 with the block's own
    fixed values (noise, bias, the same f_bar rows), predicting the withheld point with its noise."""
    import cimrgp_amd as ca
    from cimrgp_amd.Posteriors import DenseBlock
    x, y = _problem(1, 600, seed=5)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(600, 1, 2), spectral_density_obj=_kernels(ca, "mixed")[:2])
    m.fit()
    j, l = 1, 1
    a, b = (int(v) for v in m.index_set_obj.bounds[j][l])
    blk = m.posterior_obj[j].blocks[l]
    mean, var = m.leave_one_out(j)
    k = blk.kernel.with_noise(float(blk.noise.item()))
    f_bar = m._f_bar_layers[j]
    rng = np.random.default_rng(8)
    for i in rng.choice(b - a, size=8, replace=False):
        keep = torch.as_tensor(np.delete(np.arange(a, b), i), device="cuda")
        xk, yk, fk = m._x_dev[keep].contiguous(), m._y[keep].contiguous(), f_bar[keep].contiguous()
        fresh = DenseBlock(xk, k)
        fresh.fit(yk, fk, torch.zeros_like(yk), shared_bias=blk.bias.clone())
        dev.raise_if_not_pd(fresh.info)
        pm = f_bar[a + i:a + i + 1].clone()
        pv = torch.zeros(1, dtype=pm.dtype, device="cuda")
        fresh.predict(m._x_dev[a + i:a + i + 1].contiguous(), pm, pv, add_noise=True)
        bm, bv = pm.cpu().numpy()[0], float(pv.item())
        em = float(np.max(np.abs(mean[a + i] - bm)) / np.max(np.abs(bm)))
        ev = abs(var[a + i] - bv) / bv
        print("point %d: mean %.3e var %.3e (relative to the refit)" % (i, em, ev))
        assert em <= 1e-8 and ev <= 1e-8


# ---- the plugin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "ard", "matern"])
def test_plugin_leave_one_out(kind):
    import cimrgp_amd as ca
    rng = np.random.default_rng(4)
    x = rng.uniform(-2, 2, size=(300, 2)) * np.array([1.0, 2.5])
    y = np.stack([np.sin(2 * x[:, 0]) + x[:, 1], np.cos(x[:, 1])], axis=1) + 0.1 * rng.normal(size=(300, 2))
    gp = {"rbf": lambda: ca.GP_RBF(optimize=False), "ard": lambda: ca.GP_RBF(ARD=True, max_iters=30),
          "matern": lambda: ca.GP_Matern(2.5, optimize=False)}[kind]()
    gp.fit((x, y))
    mean, var = gp.leave_one_out()
    lpd = gp.loo_log_predictive_density()
    blk = gp.block
    L = np.tril(blk.lbuf[:blk.n, :blk.n].double().cpu().numpy())
    d = kinv_diag(L)
    yz = (y - gp.labels_mean) / gp.labels_std
    mz = yz - blk.alpha.double().cpu().numpy() / d[:, None]
    assert rel(mean, mz * gp.labels_std + gp.labels_mean) <= 1e-9 and rel(var, 1 / d) <= 1e-9
    assert lpd.shape == (300,) and rel(lpd, loo_log_density(yz, mz, 1 / d)) <= 1e-9
    # the variance of an observation: never below the noise
    assert var.min() >= blk.kernel.noise


# ---- one rank against two -------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    ca.dist.share_one_gpu()
    x, y = _problem(1, 1200, seed=21)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(1200, 2, 2, first_divider_power=1),
                                          spectral_density_obj=_kernels(ca, "mixed"))
    m.fit()
    out = dict()
    for j in range(3):
        out["mean%d" % j], out["var%d" % j] = m.leave_one_out(j)
    out["ll"] = np.array(m.get_loo_likelihood())
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    td.barrier()
    td.destroy_process_group()


def test_leave_one_out_two_ranks_equal_one(tmp_path):
    import torch.multiprocessing as mp
    import cimrgp_amd as ca
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    x, y = _problem(1, 1200, seed=21)
    m = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(1200, 2, 2, first_divider_power=1),
                                          spectral_density_obj=_kernels(ca, "mixed"))
    m.fit()
    for j in range(3):
        mean, var = m.leave_one_out(j)
        for g in got:
            assert rel(g["mean%d" % j], mean) <= 1e-12 and rel(g["var%d" % j], var) <= 1e-12, j
    assert np.array_equal(got[0]["ll"], got[1]["ll"]) and abs(float(got[0]["ll"]) - m.get_loo_likelihood()) <= 1e-12 * abs(float(got[0]["ll"]))
