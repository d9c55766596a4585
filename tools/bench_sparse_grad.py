"""Timing of the analytic gradient of the sparse objective (include/cimrgp_sparse_grad.h) on one GPU: FP64, device events
after warm-up, median of --reps, the routes alternating in one process, at (n, m) = (65536, 1024) and (262144, 1000),
d = 2, q = 1, FITC and VFE:
  * one SparseBlock.lml_grad call (3 + m d derivatives) against one objective evaluation (fit + log_marginal_likelihood),
    of which two-point differences spend four per step on theta alone (``*_spread_ms``: max - min over the repetitions);
  * the entry points of the call on the call's own operands: cimrgp_trsm_rows, cimrgp_trsm_rows_lt (with L_B and with
    L_u), cimrgp_wsyrk_tn, cimrgp_sparse_grad_rows, cimrgp_sparse_grad_combine, cimrgp_cov_pair_grad;
  * cimrgp_cov_pair_grad against cimrgp_cov_cross at the same shape (the same pairs and exponentials, a read of G instead
    of a write of K), with its bytes of G per second against 8 TB/s;
  * peak device memory of the call.
FP32 and several GPUs are not timed.  One JSON line per case on stdout, appended to the file named by the first argument
if given."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
from cimrgp_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()
HBM_BYTES_PER_S = 8e12
dev_name = torch.cuda.get_device_name(0)
tdt = torch.float64


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fns, reps, warmup=2, spread=None):
    """Median times (ms) of the callables, alternating, device events around each call (a call that reads back, as the
    two routes do, ends inside its events)."""
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
    if spread is not None:          # max - min of each callable's times: what a later comparison of medians can tell apart
        spread.extend(float(max(t) - min(t)) for t in ts)
    return [float(np.median(t)) for t in ts]


d, q = 2, 1
for n, m in ((65536, 1024), (262144, 1000)):
    rng = np.random.default_rng(n)
    x = rng.uniform(-2, 2, size=(n, d))
    y = (np.sin(2 * x).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    for cls in (ca.SGP_FITC, ca.SparseGP_RBF):
        g = cls(num_inducing=m, lengthscale=0.5)
        g.fit([x, y])
        k = g.kernel
        new_block = lambda: g._block(k.l, k.sf, k.noise)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        new_block().lml_grad(g._y)
        torch.cuda.synchronize()
        peak_grad = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        new_block().fit(g._y).log_marginal_likelihood()
        torch.cuda.synchronize()
        peak_fit = torch.cuda.max_memory_allocated() - base
        spread = []
        t_grad, t_theta, t_eval = timed((lambda: new_block().lml_grad(g._y), lambda: new_block().lml_grad(g._y, want_z=False),
                                         lambda: new_block().fit(g._y).log_marginal_likelihood()), args.reps, spread=spread)
        # the entry points on the call's own operands
        blk = g.block
        a0 = dev.rbf_cross(blk.x, blk.z, k.l, k.sf, cov=k.cov)
        dev.trsm_rows(blk.lu, m, blk.ws_u, a0, n)
        _, w, _ = dev.sparse_lambda(a0, n, m, k.sf, k.noise, blk.mode)
        buf = torch.empty_like(a0)
        beta, t, _ = dev.sparse_grad_rows(a0, n, m, blk.gamma, g._y, w, blk.mode, k.noise)
        bq = torch.randn((m, q), dtype=tdt, device="cuda")
        ws_scratch = torch.empty(dev.wsyrk_tn_scratch_bytes(n, m, 0, tdt), dtype=torch.uint8, device="cuda")
        c = dev.alloc_matrix(m, m, tdt, "cuda")
        pg_scratch = torch.empty(dev.cov_pair_grad_scratch_bytes(n, m, d), dtype=torch.uint8, device="cuda")
        sums = torch.zeros(2, dtype=torch.float64, device="cuda")
        dz = torch.zeros((m, d), dtype=tdt, device="cuda")

        def solve(fn, factor, ws):
            buf.copy_(a0)
            fn(factor, m, ws, buf, n)

        t_copy, t_fwd, t_lt_b, t_lt_u, t_wsyrk, t_rows, t_comb, t_pair, t_pair_sums, t_cross = timed((
            lambda: buf.copy_(a0),
            lambda: solve(dev.trsm_rows, blk.lb, blk.ws_b),
            lambda: solve(dev.trsm_rows_lt, blk.lb, blk.ws_b),
            lambda: solve(dev.trsm_rows_lt, blk.lu, blk.ws_u),
            lambda: dev.wsyrk_tn(a0, n, m, t, None, 0.0, out=c, scratch=ws_scratch),
            lambda: dev.sparse_grad_rows(a0, n, m, blk.gamma, g._y, w, blk.mode, k.noise, beta=beta, t=t),
            lambda: dev.sparse_grad_combine(a0, buf, n, m, beta, bq, w, t),
            lambda: dev.cov_pair_grad(blk.x, blk.z, a0, k.l, k.sf, sums=sums, db=dz, cov=k.cov, scratch=pg_scratch),
            lambda: dev.cov_pair_grad(blk.x, blk.z, a0, k.l, k.sf, sums=sums, want_db=False, cov=k.cov, scratch=pg_scratch),
            lambda: dev.rbf_cross(blk.x, blk.z, k.l, k.sf, out=buf, cov=k.cov)), args.reps)
        g_bytes = 8.0 * n * m
        emit({"case": "sparse_lml_grad", "device": dev_name, "dtype": "f64", "approximation": g.approximation, "n": n, "m": m,
              "d": d, "q": q, "lml_grad_ms": t_grad, "lml_grad_theta_only_ms": t_theta, "evaluation_ms": t_eval,
              "lml_grad_spread_ms": spread[0], "lml_grad_theta_only_spread_ms": spread[1], "evaluation_spread_ms": spread[2],
              "lml_grad_over_evaluation": t_grad / t_eval, "below_four_evaluations": bool(t_grad < 4 * t_eval),
              "trsm_rows_ms": t_fwd - t_copy, "trsm_rows_lt_lb_ms": t_lt_b - t_copy, "trsm_rows_lt_lu_ms": t_lt_u - t_copy,
              "wsyrk_tn_ms": t_wsyrk, "sparse_grad_rows_ms": t_rows, "sparse_grad_combine_ms": t_comb,
              "cov_pair_grad_ms": t_pair, "cov_pair_grad_sums_only_ms": t_pair_sums, "cov_cross_ms": t_cross,
              "cov_pair_grad_over_cov_cross": t_pair / t_cross, "cov_pair_grad_g_bytes_per_s": g_bytes / (t_pair * 1e-3),
              "cov_pair_grad_share_of_8_tb_s": g_bytes / (t_pair * 1e-3) / HBM_BYTES_PER_S,
              "lml_grad_peak_device_mib": peak_grad / 2.0 ** 20, "evaluation_peak_device_mib": peak_fit / 2.0 ** 20,
              "one_n_by_m_buffer_mib": a0.numel() * 8 / 2.0 ** 20})
        del g, blk, a0, buf, w, beta, t, ws_scratch, c, pg_scratch
        torch.cuda.empty_cache()
