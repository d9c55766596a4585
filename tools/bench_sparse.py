"""Timing of the sparse (inducing-point) GP pieces (include/cimrgp_sparse.h) on one GPU, device events after warm-up,
FP64, median of --reps, the new and the old route alternating in one process:
  * cimrgp_wsyrk_tn against what the library could do for the same product before it -- rows of A scaled by sqrt(w)
    with torch, transposed to m x n with torch, cimrgp_syrk_lower with K = n -- at (n, m) = (65536, 1024),
    (65536, 2048) and (262144, 1000), with n m (m + 1) flop / time against the 78.6 TF/s FP64 matrix peak;
  * SGP_FITC.fit and predict (N* = 100 000) at n = 65536 and 262144, m = 1000, d = 2, with the time of
    cimrgp_trsm_rows on the n x m operand (the same flop count as the product), cimrgp_wsyrk_tn on it, and the peak
    device memory of the fit against the n^2 elements of an exact block.
FP32 and several GPUs are not timed.  One JSON line per case on stdout, appended to the file named by the first argument
if given."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
from cimrgp_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kernel-only", action="store_true", help="only the cimrgp_wsyrk_tn cases (for a kernel trace)")
args = ap.parse_args()
dev.require_gpu()
PEAK_F64 = 78.6e12
dev_name = torch.cuda.get_device_name(0)
tdt = torch.float64


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fns, reps, warmup=2):
    """Median device times (ms) of the callables, alternating, events around each call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in ts]


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


# ---- the product -------------------------------------------------------------------------------------------------------
for n, m in ((65536, 1024), (65536, 2048), (262144, 1000)):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + m)
    a = dev.alloc_matrix(n, m, tdt, "cuda")
    a.copy_(torch.randn(a.shape, generator=gen, device="cuda", dtype=tdt))
    w = 10.0 ** (4 * torch.rand(n, generator=gen, device="cuda", dtype=tdt) - 2)
    c_new = dev.alloc_matrix(m, m, tdt, "cuda")
    c_old = dev.alloc_matrix(m, m, tdt, "cuda")
    scratch = torch.empty(dev.wsyrk_tn_scratch_bytes(n, m, 0, tdt), dtype=torch.uint8, device="cuda")
    at = dev.alloc_matrix(m, n, tdt, "cuda")

    def new():
        dev.wsyrk_tn(a, n, m, w, None, 0.0, out=c_new, scratch=scratch)

    def old():
        scaled = a[:n, :m] * torch.sqrt(w)[:, None]
        at[:m, :n].copy_(scaled.t())
        c_old.zero_()
        dev.syrk_lower(c_old, at, m, n)                  # lower(c_old) = -A^T W A

    def old_syrk_only():
        dev.syrk_lower(c_old, at, m, n)

    t_new, t_old, t_syrk = timed((new, old, old_syrk_only), args.reps)
    new(), old()
    il = torch.tril_indices(m, m, device="cuda")
    diff = float(((c_new[il[0], il[1]] + c_old[il[0], il[1]]).abs().max() / c_new[il[0], il[1]].abs().max()).item())
    flops = float(n) * m * (m + 1)
    emit({"case": "wsyrk_tn", "device": dev_name, "dtype": "f64", "n": n, "m": m, "wsyrk_tn_ms": t_new,
          "scale_transpose_syrk_lower_ms": t_old, "of_which_syrk_lower_ms": t_syrk, "old_over_new": t_old / t_new,
          "wsyrk_tn_tflops": flops / t_new / 1e9, "wsyrk_tn_share_of_f64_peak": flops / (t_new * 1e-3) / PEAK_F64,
          "scratch_mib": scratch.numel() / 2.0 ** 20, "max_rel_diff_new_old": diff})
    del a, w, c_new, c_old, scratch, at
    torch.cuda.empty_cache()

if args.kernel_only:
    sys.exit(0)

# ---- the plugin ----------------------------------------------------------------------------------------------------------
m, d, ns = 1000, 2, 100000
for n in (65536, 262144):
    rng = np.random.default_rng(n)
    x = rng.uniform(-2, 2, size=(n, d))
    y = (np.sin(2 * x).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    xs = rng.uniform(-2, 2, size=(ns, d))
    g = ca.SGP_FITC(num_inducing=m, lengthscale=0.5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_fit = wall(lambda: g.fit([x, y]), args.reps)
    peak = torch.cuda.max_memory_allocated() - base
    t_pred = wall(lambda: g.predict_with_variance(xs), args.reps)
    blk = g.block
    k = blk.kernel
    # the fit's two n m^2 steps on their own, on the fit's own operand
    abuf = dev.rbf_cross(blk.x, blk.z, k.l, k.sf, cov=k.cov)
    a0 = abuf.clone()
    w = torch.full((n,), 1.0 / k.noise, dtype=tdt, device="cuda")
    scratch = torch.empty(dev.wsyrk_tn_scratch_bytes(n, m, 1, tdt), dtype=torch.uint8, device="cuda")
    c = dev.alloc_matrix(m, m, tdt, "cuda")
    gq = torch.empty((m, 1), dtype=tdt, device="cuda")

    def trsm():
        abuf.copy_(a0)
        dev.trsm_rows(blk.lu, m, blk.ws_u, abuf, n)

    t_trsm, t_copy, t_wsyrk, t_cross = timed((trsm, lambda: abuf.copy_(a0),
                                              lambda: dev.wsyrk_tn(abuf, n, m, w, g._y, 1.0, out=c, g=gq, scratch=scratch),
                                              lambda: dev.rbf_cross(blk.x, blk.z, k.l, k.sf, out=abuf, cov=k.cov)), args.reps)
    emit({"case": "sgp_fitc", "device": dev_name, "dtype": "f64", "n": n, "m": m, "d": d, "fit_wall_ms": t_fit,
          "predict_with_variance_wall_ms": t_pred, "n_test": ns, "trsm_rows_ms": t_trsm - t_copy, "wsyrk_tn_ms": t_wsyrk,
          "cov_cross_ms": t_cross, "trsm_rows_share_of_fit": (t_trsm - t_copy) / t_fit, "wsyrk_tn_share_of_fit": t_wsyrk / t_fit,
          "fit_peak_device_mib": peak / 2.0 ** 20, "exact_block_n2_mib": 8.0 * n * n / 2.0 ** 20,
          "log_marginal_likelihood": g.log_marginal_likelihood()})
    del g, blk, abuf, a0, w, scratch, c, gq
    torch.cuda.empty_cache()
