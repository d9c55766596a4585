"""Timing of the leave-one-out pieces (include/cimrgp_loo.h) on one GPU, CUDA events after warm-up, FP64, median of
--reps, the new and the old route alternating in one process:
  * cimrgp_kinv_diag against the route that existed before it -- the n x n identity through cimrgp_trsm_rows, rows
    squared and summed -- at one block of n = 4096 / 8192 / 16384 and, batched, 128 x 2048, 64 x 4096, 16 x 8192 (the old
    route has no batched form: its blocks run one after another on the stream);
  * the FP32 error of both routes against the FP64 NumPy value on the same factor (n = 4096);
  * MultiResolutionGaussianProcess.leave_one_out() against fit() and get_predicted_mean_and_var at the training inputs on
    the 1-D chain of config 3 at N = 16384 (IndexSetUniform(N, 4, 2)), with the peak extra device memory of the call.
One JSON line per case on stdout, appended to the file named by the first argument if given."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import workloads
from cimrgp_amd import device as dev
from cimrgp_amd.Posteriors import LOO_SCRATCH_BYTES

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()
PEAK_F64 = 78.6e12
dev_name = torch.cuda.get_device_name(0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed_pair(new, old, reps, warmup=2):
    """Median device times (ms) of new() and old(), alternating, events around each call."""
    for _ in range(warmup):
        new()
        old()
    torch.cuda.synchronize()
    ts = {0: [], 1: []}
    for _ in range(reps):
        for k, fn in enumerate((new, old)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return float(np.median(ts[0])), float(np.median(ts[1]))


def wall(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def factor(n, tdt):
    x, _ = workloads.make_block(n, 2)
    xd = dev.to_device(x, tdt, "cuda")
    kbuf = dev.rbf_gram(xd, 0.5, 1.0, 0.01, lower_only=True)
    ws, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    return kbuf, ws


def old_route(kbuf, n, ws, eye, out):
    eye.zero_()
    eye[:n, :n].fill_diagonal_(1.0)
    dev.trsm_rows(kbuf, n, ws, eye, n)
    torch.sum(eye[:n, :n] * eye[:n, :n], dim=1, out=out)


# ---- diag(K^-1): one block ------------------------------------------------------------------------------------------
tdt = torch.float64
for n in (4096, 8192, 16384):
    kbuf, ws = factor(n, tdt)
    eye = dev.alloc_matrix(n, n, tdt, "cuda")
    d_new = torch.empty(n, dtype=tdt, device="cuda")
    d_old = torch.empty(n, dtype=tdt, device="cuda")
    t_new, t_old = timed_pair(lambda: dev.kinv_diag(kbuf, n, ws, LOO_SCRATCH_BYTES, out=d_new),
                              lambda: old_route(kbuf, n, ws, eye, d_old), args.reps)
    strip = min(dev.kinv_diag_scratch_bytes(n, n, tdt), LOO_SCRATCH_BYTES) // (8 * ((n + 15) // 16 * 16)) // 256 * 256
    flops = float(n) ** 3 / 3
    emit({"case": "kinv_diag", "device": dev_name, "dtype": "f64", "n": n, "batch": 1, "strip_rows": int(strip), "kinv_diag_ms": t_new,
          "identity_through_trsm_rows_ms": t_old, "new_over_old": t_new / t_old, "kinv_diag_tflops": flops / t_new / 1e9,
          "kinv_diag_share_of_f64_peak": flops / (t_new * 1e-3) / PEAK_F64,
          "max_rel_diff_new_old": float(((d_new - d_old).abs() / d_old).max().item())})
    del kbuf, ws, eye

# ---- diag(K^-1): batches ----------------------------------------------------------------------------------------------
for batch, n in ((128, 2048), (64, 4096), (16, 8192)):
    kbuf, ws = factor(n, tdt)
    ld = kbuf.stride(0)
    karena = kbuf[:n].unsqueeze(0).repeat(batch, 1, 1).contiguous()
    ws_arena = ws.view(torch.uint8).reshape(1, -1).repeat(batch, 1).contiguous()
    eye = dev.alloc_matrix(n, n, tdt, "cuda")
    d_new = torch.empty((batch, n), dtype=tdt, device="cuda")
    d_old = torch.empty((batch, n), dtype=tdt, device="cuda")

    def old_all():
        for b in range(batch):
            old_route(karena[b], n, ws_arena[b], eye, d_old[b])
    t_new, t_old = timed_pair(lambda: dev.kinv_diag_batched(karena, n, ws_arena, LOO_SCRATCH_BYTES, out=d_new), old_all, args.reps)
    flops = batch * float(n) ** 3 / 3
    emit({"case": "kinv_diag_batched", "device": dev_name, "dtype": "f64", "n": n, "batch": batch, "kinv_diag_ms": t_new,
          "identity_through_trsm_rows_ms": t_old, "old_route": "block after block on one stream", "new_over_old": t_new / t_old,
          "kinv_diag_tflops": flops / t_new / 1e9, "kinv_diag_share_of_f64_peak": flops / (t_new * 1e-3) / PEAK_F64,
          "max_rel_diff_new_old": float(((d_new - d_old).abs() / d_old).max().item())})
    del kbuf, ws, karena, ws_arena, eye

# ---- FP32 error of both routes ------------------------------------------------------------------------------------------
n = 4096
kbuf, ws = factor(n, torch.float32)
L = np.tril(kbuf[:n, :n].double().cpu().numpy())
import scipy.linalg as sla
want = (sla.solve_triangular(L, np.eye(n), lower=True) ** 2).sum(axis=0)
eye = dev.alloc_matrix(n, n, torch.float32, "cuda")
d_old = torch.empty(n, dtype=torch.float32, device="cuda")
old_route(kbuf, n, ws, eye, d_old)
d_new = dev.kinv_diag(kbuf, n, ws, LOO_SCRATCH_BYTES)
emit({"case": "kinv_diag_fp32_error", "device": dev_name, "n": n,
      "kinv_diag_max_rel_err": float(np.max(np.abs(d_new.double().cpu().numpy() / want - 1))),
      "identity_through_trsm_rows_max_rel_err": float(np.max(np.abs(d_old.double().cpu().numpy() / want - 1)))})
del kbuf, ws, eye

# ---- the model ------------------------------------------------------------------------------------------------------
import cimrgp_amd as ca

xm, ym, _ = workloads.make_chain_1d(16384, 2)
ells = workloads.chain_length_scales(5, 1)
nm = xm.shape[0]
kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
model = ca.MultiResolutionGaussianProcess([xm, ym], index_set_obj=ca.IndexSetUniform(nm, 4, 2), spectral_density_obj=kernels)
t_fit = wall(model.fit, args.reps)
iset = ca.IndexSetUniform(nm, 4, 2)
t_pred = wall(lambda: model.get_predicted_mean_and_var(xm, iset), args.reps)
rec = {"case": "model", "model": "config3_chain_n16384", "device": dev_name, "n": nm, "layers": 5, "fit_ms": t_fit,
       "get_predicted_mean_and_var_at_training_inputs_ms": t_pred}
for j in (0, 4):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rec["leave_one_out_layer%d_ms" % j] = wall(lambda: model.leave_one_out(j), args.reps)
    rec["leave_one_out_layer%d_peak_extra_mib" % j] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
rec["loo_finest_over_fit"] = rec["leave_one_out_layer4_ms"] / t_fit
rec["loo_finest_over_predict"] = rec["leave_one_out_layer4_ms"] / t_pred
rec["loo_likelihood_finest"] = float(model.get_loo_likelihood())
emit(rec)
