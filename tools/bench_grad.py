"""Timing of the predictive-gradient pieces (include/cimrgp_grad.h) on one GPU, CUDA events after warm-up, FP64:
  * cimrgp_trsm_rows_lt (B <- B L^-1) against cimrgp_trsm_rows (B <- B L^-T) at n = 8192, m in {1024, 8192};
  * cimrgp_cov_predict_grad (RBF, d = 1, q = 2) at n = 8192, ns = 2048: mean only, variance only, both;
  * MultiResolutionGaussianProcess.predictive_gradients against one get_predicted_mean_and_var on the bench-sized
    block (bench.py's flagship: one block of n = 8192, ns = 2048, q = 2) and on the 1-D chain of config 3 at
    N = 16384 (IndexSetUniform(N, 4, 2)).
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

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()
PEAK_F64 = 78.6e12


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps, warmup=2):
    """Median device time (ms) of fn over reps, events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall(fn, reps, warmup=1):
    """Median wall time (ms): host calls that read back to the host."""
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


tdt = torch.float64
dev_name = torch.cuda.get_device_name(0)

# ---- the row solves -------------------------------------------------------------------------------------------------
n = 8192
x, y = workloads.make_block(n, 2)
xd = dev.to_device(x, tdt, "cuda")
kbuf = dev.rbf_gram(xd, 0.5, 1.0, 0.01, lower_only=True)
ws, info = dev.potrf(kbuf, n)
assert int(info.item()) == 0
for m in (1024, 8192):
    b0 = torch.randn((m, kbuf.stride(0)), dtype=tdt, device="cuda")
    b = b0.clone()
    t_fwd = timed(lambda: dev.trsm_rows(kbuf, n, ws, b, m), args.reps)
    t_bwd = timed(lambda: dev.trsm_rows_lt(kbuf, n, ws, b, m), args.reps)
    flops = float(m) * n * n
    emit({"case": "row_solves", "device": dev_name, "n": n, "m": m, "trsm_rows_ms": t_fwd, "trsm_rows_lt_ms": t_bwd,
          "lt_over_forward": t_bwd / t_fwd, "trsm_rows_lt_tflops": flops / t_bwd / 1e9,
          "trsm_rows_lt_share_of_f64_peak": flops / (t_bwd * 1e-3) / PEAK_F64})

# ---- the contraction ------------------------------------------------------------------------------------------------
ns = 2048
xs = dev.to_device(workloads.block_test_points(ns), tdt, "cuda")
alpha = torch.randn((n, 2), dtype=tdt, device="cuda")
beta = dev.alloc_matrix(ns, n, tdt, "cuda").normal_()
mg = torch.zeros((ns, 1, 2), dtype=tdt, device="cuda")
vg = torch.zeros((ns, 1), dtype=tdt, device="cuda")
rec = {"case": "cov_predict_grad", "device": dev_name, "n": n, "ns": ns, "d": 1, "q": 2, "cov": "rbf"}
rec["mean_ms"] = timed(lambda: dev.cov_predict_grad(xd, alpha, xs, 0.5, 1.0, mean_grad=mg), args.reps)
rec["var_ms"] = timed(lambda: dev.cov_predict_grad(xd, alpha, xs, 0.5, 1.0, beta=beta, var_grad=vg), args.reps)
rec["both_ms"] = timed(lambda: dev.cov_predict_grad(xd, alpha, xs, 0.5, 1.0, beta=beta, mean_grad=mg, var_grad=vg), args.reps)
rec["var_beta_read_gbs"] = ns * n * 8 / (rec["var_ms"] * 1e-3) / 1e9
emit(rec)
del kbuf, ws, b0, b, beta

# ---- the model ----------------------------------------------------------------------------------------------------
import cimrgp_amd as ca

for label, (xm, ym, xsm, res, ells) in {
        "flagship_block_n8192": (x, y, workloads.block_test_points(ns), 0, [0.5]),
        "config3_chain_n16384": workloads.make_chain_1d(16384, 2) + (4, workloads.chain_length_scales(5, 1))}.items():
    nm = xm.shape[0]
    kernels = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
    model = ca.MultiResolutionGaussianProcess([xm, ym], index_set_obj=ca.IndexSetUniform(nm, res, 2), spectral_density_obj=kernels)
    model.fit()
    iset = ca.IndexSetUniform(xsm.shape[0], res, 2)
    t_pred = wall(lambda: model.get_predicted_mean_and_var(xsm, iset), args.reps)
    t_grad = wall(lambda: model.predictive_gradients(xsm, iset), args.reps)
    emit({"case": "model", "model": label, "device": dev_name, "n": nm, "ns": int(xsm.shape[0]), "layers": res + 1,
          "get_predicted_mean_and_var_ms": t_pred, "predictive_gradients_ms": t_grad, "grad_over_predict": t_grad / t_pred})
