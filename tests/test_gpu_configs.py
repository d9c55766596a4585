"""BASELINE.json configs 3, 4 and 5 under ``pytest -m gpu``.

  config 3  1-D, 5-layer residual chain: against the oracle at N = 8192, and at the full
            N = 65536 (31 blocks) through size-independent properties per block;
  config 4  2-D inputs in Hilbert order, 5 resolutions, hierarchy started at a layer whose
            blocks fit (root-block policy ``first_divider_power=3``: 8, 16, 32, 64, 128
            regions): against the oracle at reduced N, single process and sharded over 2 ranks;
  config 5  one n = 16384 block, FP64 and FP32 posteriors against the CPU oracle, ``info > 0``
            where FP32 loses positive definiteness.
"""
import os
import socket

import numpy as np
import pytest

import oracle
import workloads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / (np.max(np.abs(b)) + 1e-300))


def _relerr_elem(a, b):
    """Element-wise relative error max_i |a_i - b_i| / |b_i|: the strict reading of north_star's "1e-5 relative"
    for the variance, whose entries span orders of magnitude (``_relerr`` is relative to the array's largest)."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


def _oracle_chain(x, y, xs, bounds, tbounds, ells, noise):
    xn, _, mu, sd = oracle.normalize_inputs(x)
    specs = [oracle.DenseLayerSpec(l, 1.0, noise) for l in ells]
    om, f_bar = oracle.mrgp_fit(xn, y, bounds, specs)
    omean, ovar = oracle.mrgp_predict(xn, om, specs, (xs - mu) / sd, tbounds)
    return omean, ovar, f_bar


# ------------------------------------------------------------------------------------ config 3
def test_config3_chain_n8192_matches_oracle(ca):
    """The config-3 recipe (IndexSetUniform(N, 4, 2): 1+2+4+8+16 = 31 blocks, l_j = 2^-j, fixed
    noise) at N = 8192, where the CPU oracle finishes in seconds."""
    n, res = 8192, 4
    x, y, xs = workloads.make_chain_1d(n)
    ells = workloads.chain_length_scales(res + 1, 1)
    kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2),
                                              spectral_density_obj=kernels)
    model.fit()
    idx_t = ca.IndexSetUniform(xs.shape[0], res, 2)
    mean, var = model.get_predicted_mean_and_var(xs, idx_t)
    omean, ovar, f_bar = _oracle_chain(x, y, xs, oracle.index_bounds_uniform(n, res, 2),
                                       oracle.index_bounds_uniform(xs.shape[0], res, 2), ells, 0.01)
    assert sum(model.n_regions) == 31
    assert _relerr(mean, omean) < 1e-5 and _relerr(var, ovar) < 1e-5          # north_star bar, relative to the array's largest
    assert _relerr_elem(var, ovar) < 1e-5                                      # ... and element by element
    assert _relerr(mean, omean) < 1e-7 and _relerr(var, ovar) < 1e-6
    assert _relerr(model._f_bar_final.cpu().numpy(), f_bar) < 1e-7


def _gram_times(x, v, ell, sf, chunk=4096):
    """K(x, x) v by an independent route (torch broadcasting, chunked): the checker of K alpha = r."""
    out = torch.empty_like(v)
    for i0 in range(0, x.shape[0], chunk):
        d2 = torch.zeros((min(chunk, x.shape[0] - i0), x.shape[0]), dtype=x.dtype, device=x.device)
        for k in range(x.shape[1]):
            diff = x[i0:i0 + chunk, k][:, None] - x[:, k][None, :]
            d2 += diff * diff
        out[i0:i0 + chunk] = (sf * torch.exp(d2 * (-0.5 / (ell * ell)))) @ v
    return out


def _check_block_properties(model, tol_solve=1e-7):
    """Size-independent properties of every fitted block: (K + noise I) alpha = r with K rebuilt by
    an independent route, the residual-chain identity f_bar_{j+1} - f_bar_j = r - noise alpha + bias
    on the block's rows, a clean LAPACK ``info``."""
    worst = 0.0
    for j in range(model.n_layers):
        f_in = model._f_bar_layers[j]
        f_out = model._f_bar_layers[j + 1] if j + 1 < model.n_layers else model._f_bar_final
        k = model.spectral_density_obj[j]
        for l, (a, b) in enumerate(model.index_set_obj.bounds[j]):
            a, b = int(a), int(b)
            blk = model.posterior_obj[j].blocks[l]
            assert int(blk.info.item()) == 0
            r = model._y[a:b] - f_in[a:b] - blk.bias
            noise = float(blk.noise.item())
            lhs = _gram_times(model.x[j][l], blk.alpha, k.l, k.sf) + noise * blk.alpha
            err = float((lhs - r).abs().max() / r.abs().max())
            worst = max(worst, err)
            assert err < tol_solve, (j, l, err)
            chain = (f_out[a:b] - f_in[a:b]) - (r - noise * blk.alpha + blk.bias)
            assert float(chain.abs().max()) < 1e-9, (j, l)
    return worst


def test_config3_full_size_n65536_properties(ca):
    """BASELINE configs[2] at full size: N = 65536, 5 layers, 31 blocks (65536 ... 4096 rows) on one
    GPU.  No N^3 CPU reference exists at this size: every block is checked through K alpha = r
    (K rebuilt by torch), the chain identity, finite means and positive, bounded variances."""
    n, res = 65536, 4
    x, y, xs = workloads.make_chain_1d(n)
    ells = workloads.chain_length_scales(res + 1, 1)
    kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, res, 2),
                                              spectral_density_obj=kernels)
    model.fit()
    assert [len(b) for b in model.index_set_obj.bounds] == [1, 2, 4, 8, 16]
    _check_block_properties(model)
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], res, 2), include_noise=False)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    # latent variance: a sum over 5 layers of sf - |L^-1 k*|^2, each in [0, sf] up to rounding
    assert var.min() > -1e-8 and var.max() <= 5.0 + 1e-8
    # the model explains the data to about the noise level it was given (sd 0.1)
    rmse = float(np.sqrt(np.mean((model._f_bar_final.cpu().numpy() - y) ** 2)))
    assert 0.02 < rmse < 0.2, rmse
    del model
    torch.cuda.empty_cache()


def test_factorisation_checksum_three_panel_groups_n18432(ca):
    """N = 18432: the far part of the trailing matrix exceeds 16384 rows at the start, so the first
    groups update it once per THREE panels (K = 768), later ones per two, the tail per panel
    (potrf.hip group_size).  Checksum K v = L (L^T v) and LAPACK on the leading minor."""
    dev = ca.device
    rng = np.random.default_rng(18432)
    n = 18432
    x = np.sort(rng.uniform(-2.0, 2.0, size=(n, 1)), axis=0)
    ell, sf2, noise = 0.05, 1.0, 0.01
    xd = dev.to_device(x, torch.float64, "cuda")
    kbuf = dev.rbf_gram(xd, ell, sf2, noise, lower_only=False)
    v = torch.from_numpy(rng.normal(size=(n, 3))).cuda()
    rhs = kbuf[:n, :n] @ v
    _, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    lmat = torch.tril(kbuf[:n, :n])
    assert float((lmat @ (lmat.t() @ v) - rhs).abs().max() / rhs.abs().max()) < 1e-11
    lref, _ = oracle.potrf_lower(oracle.rbf_gram(x[:1536], None, ell, sf2, noise))
    assert _relerr(lmat[:1536, :1536].cpu().numpy(), lref) < 1e-9
    del kbuf, lmat
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ config 4
def _config4_problem(ca, n, res=4, power=3):
    x, y, xs = workloads.make_chain_2d(n, order=ca.space_filling_order)
    ells = workloads.chain_length_scales(res + 1, 2, ell0=0.7)
    return x, y, xs, ells


def test_config4_reduced_2d_five_layers_matches_oracle(ca):
    """BASELINE configs[3] at reduced N: 2-D inputs in Hilbert order, 5 resolutions with 8, 16, 32,
    64, 128 regions (the hierarchy starts where blocks fit one GPU: ``first_divider_power=3``),
    against the oracle on the same arrays."""
    n, res, power = 8192, 4, 3
    x, y, xs, ells = _config4_problem(ca, n)
    ns = xs.shape[0]
    idx = ca.IndexSetUniform(n, res, 2, first_divider_power=power)
    idx_t = ca.IndexSetUniform(ns, res, 2, first_divider_power=power)
    assert idx.n_regions_per_layer() == [8, 16, 32, 64, 128]
    kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=kernels)
    model.fit()
    mean, var = model.get_predicted_mean_and_var(xs, idx_t)
    omean, ovar, f_bar = _oracle_chain(x, y, xs, oracle.index_bounds_uniform(n, res, 2, power),
                                       oracle.index_bounds_uniform(ns, res, 2, power), ells, 0.01)
    assert _relerr(mean, omean) < 1e-5 and _relerr(var, ovar) < 1e-5          # north_star bar, relative to the array's largest
    assert _relerr_elem(var, ovar) < 1e-5                                      # ... and element by element
    assert _relerr(mean, omean) < 1e-7 and _relerr(var, ovar) < 1e-6
    assert _relerr(model._f_bar_final.cpu().numpy(), f_bar) < 1e-7
    # without an index set the reference predicts from THE root region (MRGP.py:726-755): undefined here
    with pytest.raises(ValueError):
        model.get_predicted_mean(xs)
    # data-dependent noise (the plugin's 1 % rule per region) on the same hierarchy
    model2 = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx,
                                               spectral_density_obj=[ca.RBFKernel(l=l, sf=1.0) for l in ells])
    model2.fit()
    mean2, var2 = model2.get_predicted_mean_and_var(xs, idx_t)
    omean2, ovar2, _ = _oracle_chain(x, y, xs, oracle.index_bounds_uniform(n, res, 2, power),
                                     oracle.index_bounds_uniform(ns, res, 2, power), ells, None)
    assert _relerr(mean2, omean2) < 1e-6 and _relerr(var2, ovar2) < 1e-5


def _rank_worker(rank, world, port, out_dir, case):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.distributed as td
    import cimrgp_amd as ca
    import workloads
    # ranks share the one GPU of the box: gloo carries the device tensors; on a multi-GPU node the
    # same code runs with backend "nccl" (RCCL), one GPU per rank (bench.py --gpus N)
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    ca.dist.share_one_gpu()              # two processes on ONE card: each within four streams (cimrgp_amd/dist.py)
    out = dict()
    if case == "config4":
        n, res, power = 4096, 4, 3
        x, y, xs = workloads.make_chain_2d(n, order=ca.space_filling_order)
        ells = workloads.chain_length_scales(res + 1, 2, ell0=0.7)
        idx = ca.IndexSetUniform(n, res, 2, first_divider_power=power)
        model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx,
                                                  spectral_density_obj=[ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells])
        model.fit()
        mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], res, 2, first_divider_power=power))
        out = dict(mean=mean, var=var, f_bar=model._f_bar_final.cpu().numpy(),
                   owned=np.array([len(model._owned(j)) for j in range(res + 1)]))
    elif case == "nonpd":
        # layer 1 has two regions, one per rank.  Rank 1 gives its block a negative "noise" (K - 0.5 I
        # is indefinite, deterministically); rank 0's block is healthy.  BOTH ranks must raise -- the
        # owner with LAPACK's leading-minor message, the other one instead of hanging in the all-reduce.
        n = 256
        x = np.linspace(0.0, 1.0, n)[:, None]
        y = np.hstack([np.sin(4 * x), np.cos(3 * x)])
        model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(n, 1, 2),
                                                  spectral_density_obj=[ca.RBFKernel(l=1.0, sf=1.0, noise=0.05),
                                                                        ca.RBFKernel(l=0.5, sf=1.0, noise=(-0.5 if rank == 1 else 0.05))])
        owner = model.owner[1].tolist()
        try:
            model.fit()
            raised = "none"
        except np.linalg.LinAlgError as exc:
            raised = str(exc)
        out = dict(raised=np.array(raised), owner=np.array(owner))
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    td.barrier()
    td.destroy_process_group()


def _spawn(case, tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path), case), nprocs=2, join=True)
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]


def test_config4_sharded_over_two_ranks(ca, tmp_path):
    """The config-4 hierarchy with its blocks sharded over 2 ranks (per-layer residual all-reduce,
    one fused [mean | var] reduce): both ranks hold the single-process oracle's result."""
    g0, g1 = _spawn("config4", tmp_path)
    n, res, power = 4096, 4, 3
    x, y, xs, ells = _config4_problem(ca, n)
    omean, ovar, f_bar = _oracle_chain(x, y, xs, oracle.index_bounds_uniform(n, res, 2, power),
                                       oracle.index_bounds_uniform(xs.shape[0], res, 2, power), ells, 0.01)
    for g in (g0, g1):
        assert _relerr(g["mean"], omean) < 1e-7
        assert _relerr(g["var"], ovar) < 1e-6
        assert _relerr(g["f_bar"], f_bar) < 1e-7
    assert g0["owned"].tolist() == [4, 8, 16, 32, 64] and g1["owned"].tolist() == [4, 8, 16, 32, 64]


def test_config4_full_size_n262144_properties(ca):
    """BASELINE configs[3] at full size on ONE GPU: 2-D, N = 262144, 5 resolutions of 8 ... 128 regions (248
    blocks of 32768 ... 2048 points, ~130 GiB of factors).  No N^3 CPU reference exists at this size: every
    block is checked through (K + noise I) alpha = r with K rebuilt by torch, the residual-chain identity and a
    clean ``info``; means finite, latent variances within [0, 5 sf]."""
    n, res, power = 262144, 4, 3
    x, y, xs, ells = _config4_problem(ca, n)
    idx = ca.IndexSetUniform(n, res, 2, first_divider_power=power)
    assert idx.n_regions_per_layer() == [8, 16, 32, 64, 128]
    kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=kernels)
    model.fit()
    _check_block_properties(model)
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(xs.shape[0], res, 2, first_divider_power=power),
                                                 include_noise=False)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert var.min() > -1e-8 and var.max() <= 5.0 + 1e-8
    rmse = float(np.sqrt(np.mean((model._f_bar_final.cpu().numpy() - y) ** 2)))
    assert 0.02 < rmse < 0.3, rmse
    del model
    torch.cuda.empty_cache()


def _run_bench(extra, env_extra=None, timeout=900):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(sk.getsockname()[1])
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, env=env, cwd=root, capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_config4_two_ranks_prints_one_checked_line():
    """``bench.py --config 4 --gpus 2 --n 8192``: the multi-rank entry point of BASELINE configs[3].  Ranks are
    started by bench.py itself before any GPU call; here they share the one card and gloo carries the reduces
    (CIMRGP_BENCH_REHEARSAL), the driver's node runs the same code under nccl = RCCL.  Rank 0 prints ONE line
    with per-layer times, blocks per rank and, at this size, parity against the CPU oracle."""
    rec = _run_bench(["--config", "4", "--gpus", "2", "--n", "8192", "--steps", "1", "--warmup", "1"],
                     {"CIMRGP_BENCH_REHEARSAL": "gloo"})
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong" and rec["unit"] == "posteriors/s" and rec["value"] > 0
    assert rec["config"]["regions_per_layer"] == [8, 16, 32, 64, 128]
    assert rec["config"]["blocks_per_rank"] == [[4, 8, 16, 32, 64], [4, 8, 16, 32, 64]]
    assert len(rec["layer_fit_ms"]) == 5 and rec["fit_s"] > 0 and rec["predict_s"] > 0
    assert rec["parity_ok"] is True and rec["parity_rel_err_mean"] < 1e-7 and rec["parity_rel_err_var_elementwise"] < 1e-5


def test_bench_weak_scaling_two_ranks_reduce_is_exact():
    """``bench.py --gpus 2`` (the driver's weak-scaling command; here two ranks share the card under gloo): one line,
    two posteriors per step, and the asynchronously started reduce of the fused [mean | var] buffer returns rank
    0's slice bit for bit (the other ranks contribute zeros there; the buffer is zeroed every step)."""
    rec = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--full"], {"CIMRGP_BENCH_REHEARSAL": "gloo"})
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["value"] > 0
    assert rec["config"]["backend"] == "gloo" and rec["config"]["rows_queues"] == 1
    assert rec["reduce_selfcheck_max_abs_diff"] == 0.0


def test_bench_step_under_rccl_world_of_one():
    """The real bench step with backend nccl (= RCCL) initialised and the fused [mean | var] buffer reduced
    through it unconditionally -- the only RCCL evidence obtainable on one GPU -- beside the plain run, with
    the carried rows on two queues (the multi-GPU default) and on one."""
    plain = _run_bench(["--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--full"])
    rccl2 = _run_bench(["--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--full", "--nccl-world1"])
    rccl1 = _run_bench(["--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--full", "--nccl-world1", "--rows-queues", "1"])
    print("ms_per_step  plain %.3f | nccl world 1, two rows queues %.3f | one rows queue %.3f"
          % (plain["ms_per_step"], rccl2["ms_per_step"], rccl1["ms_per_step"]))
    # round 5: the step's collective is the C ABI's (cimrgp_allreduce_sum) on the step's own solve queue -- no RCCL stream of
    # torch's in the process (the fifth queue that cost the pipelined step its gain in round 4); control plane gloo
    assert plain["config"]["backend"] == "none" and rccl2["config"]["backend"].startswith("rccl through the C ABI")
    assert rccl2["config"]["rows_queues"] == 2 and rccl1["config"]["rows_queues"] == 1
    # a live RCCL communicator must not disturb the step: within 5 % of the plain run (profiles/r05_rccl_world_of_one.jsonl: 1 %)
    assert rccl2["ms_per_step"] < 1.05 * plain["ms_per_step"]
    assert rccl2["reduce_selfcheck_max_abs_diff"] == 0.0
    # the timed step is ONE C call; the collective is started at its end and hidden behind the next step: a step that
    # waits for it inside (drained_step_ms) is reported beside the headline and may not cost more than 1 ms extra
    assert plain["reduce_overlapped"] is False and plain["drained_step_ms"] is None
    assert rccl2["reduce_overlapped"] is True and rccl2["drained_step_ms"] < rccl2["ms_per_step"] + 1.0
    assert "cimrgp_block_posterior" in plain["step_is"]


def test_bench_falls_back_to_torch_nccl_when_the_c_abi_communicator_fails():
    """bench.py's N > 1 step creates the C ABI's RCCL communicator on every rank; if that fails on any of them (it has never
    seen more than one GPU) all ranks agree -- over the gloo control plane -- to reduce through torch.distributed's nccl
    instead, so that a scaling run still yields a line.  Exercised here with a simulated failure in a world of one."""
    rec = _run_bench(["--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--full", "--nccl-world1"], env_extra={"CIMRGP_BENCH_FAIL_COMM": "1"})
    assert rec["config"]["backend"].startswith("nccl (fallback")
    assert rec["reduce_overlapped"] is True and rec["reduce_selfcheck_max_abs_diff"] == 0.0
    assert rec["value"] > 0


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain ``bench.py`` run (no --full) prints the headline fields only, and ``--dump-outputs`` writes what the last
    timed step computed -- mean, variance and alpha = K^-1 r of the seeded block -- which the CPU oracle reproduces."""
    steps = 3
    rec = _run_bench(["--steps", str(steps), "--warmup", "1", "--n", "2048", "--dump-outputs", str(tmp_path)])
    assert rec["steps"] == steps and rec["unit"] == "posteriors/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["value"] == pytest.approx(1e3 / rec["ms_per_step"])
    assert not {"roofline", "stage_ms", "cpu_baseline", "parity_ok", "reduce_selfcheck_max_abs_diff"} & set(rec)
    n, ns, q = 2048, 512, 2
    got = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("mean", "var", "alpha")}
    assert got["mean"].shape == (ns, q) and got["var"].shape == (ns,) and got["alpha"].shape == (n, q)
    assert all(a.dtype == np.float64 for a in got.values())
    x, y = workloads.make_block(n, q, 1234)
    xs = workloads.block_test_points(ns)
    fit = oracle.block_fit(x, y, 0.1, 1.0, 0.01)
    omean, ovar = oracle.block_predict(x, fit, xs, 0.1, 1.0, True)
    assert _relerr(got["mean"], omean) < 1e-8 and _relerr_elem(got["var"], ovar) < 1e-5
    assert _relerr(got["alpha"], fit["alpha"]) < 1e-8


def test_c_abi_collective_world_of_one(ca):
    """The boundary's own collective (include/cimrgp.h: cimrgp_comm_unique_id / cimrgp_comm_create /
    cimrgp_allreduce_sum), ctypes only, no torch.distributed: a world of one on this GPU reduces the fused
    [mean | var] buffer of a block's posterior in place -- the sum over one rank is the buffer itself -- in both
    precisions, stream-ordered behind the kernels that fill it."""
    from cimrgp_amd import _lib
    dev = ca.device
    comm = _lib.Comm(1, 0, _lib.Comm.unique_id())
    try:
        for tdt, code in ((torch.float64, _lib.F64), (torch.float32, _lib.F32)):
            n, ns, q = 700, 130, 2
            x, y = workloads.make_block(n, q)
            xs = workloads.block_test_points(ns)
            xd, yd, xsd = (dev.to_device(a, tdt, "cuda") for a in (x, y, xs))
            kbuf, wbuf = dev.alloc_matrix(n, n, tdt, "cuda"), dev.alloc_matrix(ns + q, n, tdt, "cuda")
            ws = dev.potrf_workspace(n, tdt, "cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            fused = torch.zeros(ns * (q + 1), dtype=tdt, device="cuda")
            mean, var = fused[:ns * q].view(ns, q), fused[ns * q:]
            alpha, z = torch.empty((n, q), dtype=tdt, device="cuda"), torch.empty((n, q), dtype=tdt, device="cuda")
            dev.block_posterior(xd, yd, xsd, 0.3, 1.0, 0.05, kbuf, wbuf, ws, info, alpha, z, mean, var)
            before = fused.clone()
            comm.allreduce_sum(code, fused.data_ptr(), fused.numel(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert int(info.item()) == 0
            assert torch.equal(fused, before) and bool(torch.isfinite(fused).all())
    finally:
        comm.close()


def test_non_pd_block_raises_on_every_rank(ca, tmp_path):
    g0, g1 = _spawn("nonpd", tmp_path)
    assert g0["owner"].tolist() == [0, 1]
    assert "not positive definite" in str(g0["raised"]) and "another rank" in str(g0["raised"])
    assert "not positive definite" in str(g1["raised"]) and "leading minor" in str(g1["raised"])


# ------------------------------------------------------------------------------------ config 5
def _posterior(dev, x, y, xs, ell, sf2, noise, tdt):
    n, ns = x.shape[0], xs.shape[0]
    xd, yd, xsd = (dev.to_device(a, tdt, "cuda") for a in (x, y, xs))
    kbuf = dev.rbf_gram(xd, ell, sf2, noise, lower_only=True)
    ws, info = dev.potrf(kbuf, n)
    alpha = yd.clone()
    z = dev.potrs(kbuf, n, ws, alpha, want_z=True)
    w = dev.rbf_cross(xsd, xd, ell, sf2)
    dev.trsm_rows(kbuf, n, ws, w, ns)
    mean = torch.zeros((ns, y.shape[1]), dtype=tdt, device="cuda")
    var = torch.zeros(ns, dtype=tdt, device="cuda")
    dev.predict_from_w(w, ns, n, z, sf2, 0.0, None, mean, var)
    return int(info.item()), mean.double().cpu().numpy(), var.double().cpu().numpy()


def test_config5_n16384_fp64_and_fp32_against_oracle(ca):
    """BASELINE configs[4]: one n = 16384 block.  FP64 posterior against the CPU oracle (north_star
    bar 1e-5), FP32 against the SAME oracle (reported accuracy, loose bars), and LAPACK-style
    ``info > 0`` where FP32 loses positive definiteness (noise 1e-4)."""
    dev = ca.device
    n, ns, q = 16384, 1024, 2
    x, y = workloads.make_block(n, q)
    xs = workloads.block_test_points(ns)
    ell, sf2, noise = 0.1, 1.0, 0.01
    fit = oracle.block_fit(x, y, ell, sf2, noise)                      # ~1 min of host BLAS
    omean, ovar = oracle.block_predict(x, fit, xs, ell, sf2, True)
    i64, m64, v64 = _posterior(dev, x, y, xs, ell, sf2, noise, torch.float64)
    assert i64 == 0
    assert _relerr(m64, omean) < 1e-5 and float(np.max(np.abs(v64 - ovar))) < 1e-5 * sf2     # north_star bar
    assert _relerr_elem(v64, ovar) < 1e-5                                                    # element by element (min var ~1e-7)
    assert _relerr(m64, omean) < 1e-8 and float(np.max(np.abs(v64 - ovar))) < 1e-9
    i32, m32, v32 = _posterior(dev, x, y, xs, ell, sf2, noise, torch.float32)
    assert i32 == 0
    # FP32 is NOT within north_star's 1e-5 here (cond(K) ~ sf2 n / noise ~ 1e6 eats the digits);
    # these bars record what it does deliver at this conditioning
    assert _relerr(m32, omean) < 2e-2
    assert float(np.max(np.abs(v32 - ovar))) < 1e-4 * sf2
    i32_bad, _, _ = _posterior(dev, x, y, xs, ell, sf2, 1e-4, torch.float32)
    assert i32_bad > 0
    i64_ok, _, _ = _posterior(dev, x, y, xs, ell, sf2, 1e-4, torch.float64)
    assert i64_ok == 0


def test_bench_launches_its_own_ranks(tmp_path):
    """``python bench.py --gpus 2`` with WORLD_SIZE unset starts two ranks itself (before any GPU
    call in the parent) and rank 0 prints ONE JSON line with n_gpus == 2.  On this one-GPU box the
    ranks share the card and gloo carries the reduce (CIMRGP_BENCH_REHEARSAL); the driver's
    multi-GPU runs use nccl = RCCL with one GPU per rank."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CIMRGP_BENCH_REHEARSAL"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--n", "2048", "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["scaling"] == "weak" and rec["unit"] == "posteriors/s"
    assert rec["value"] > 0 and "roofline" in rec and "cpu_baseline" not in rec


def test_rccl_backend_initialises_and_reduces():
    """Backend "nccl" (= RCCL) with a world of one, bound to the device as bench.py binds it, reducing through
    cimrgp_amd.dist -- in a process of its own (two ranks cannot share a GPU under RCCL: the 2-rank tests
    above use gloo)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(sk.getsockname()[1])
    env["MASTER_ADDR"] = "127.0.0.1"
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "nccl_selftest.py")], env=env, cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "nccl world 1 ok 66.0 1.5" in out.stdout
