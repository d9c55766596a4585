"""Timing of the variational sparse GP (include/cimrgp_svgp.h) on one GPU: FP64, device events after warm-up, median of
--reps, the variants alternating in one process, at (n, m) = (65536, 100) and (65536, 1000), d = 2, q = 1:
  * cimrgp_svgp_rows (Student-t and Gaussian, every output wanted) against cimrgp_sparse_tail (mean and variance) on the
    same two operands A and W: the same row walk, plus the 20 nodes per row;
  * cimrgp_svgp_moments against cimrgp_wsyrk_tn with r on the same operand: the same kernels but for the weighting of r;
  * one SVGPBlock.elbo_grad against one SparseBlock('vfe').lml_grad(want_z=False) on the same data.
The ratios at m = 1000 are judged against 1.10 (``within_1_10``); at m = 100 they are reported.  FP32 and several GPUs are
not timed.  One JSON line per case on stdout, appended to the file named by the first argument if given."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
from cimrgp_amd import device as dev
from cimrgp_amd import device_svgp as devs
from cimrgp_amd.SVGP import hermite_nodes

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()
dev_name = torch.cuda.get_device_name(0)
tdt = torch.float64


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fns, reps, warmup=2):
    """Median times (ms) of the callables, alternating, device events around each call."""
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


d, q, n = 2, 1, 65536
for m in (100, 1000):
    rng = np.random.default_rng(m)
    x = rng.uniform(-2, 2, size=(n, d))
    y = (np.sin(2 * x).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    y[::17] += 3.0
    xd, yd = dev.to_device(x, tdt, "cuda"), dev.to_device(y, tdt, "cuda")
    zd = xd[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    ell, lin = np.array([0.5, 0.7]), np.array([0.3, 0.2])
    noise = 0.05
    svgp = lambda: ca.SVGPBlock(xd, zd, ca.RBFKernel(l=1.0, sf=1.0), "student_t", 3.0, noise, 0.01, 1e-6, lengthscales=ell, linear=lin)
    vfe = lambda: ca.SparseBlock(xd, zd, ca.RBFKernel(l=1.0, sf=1.0, noise=noise), "vfe", 1e-6 + 0.01, lengthscales=ell, linear=lin)
    # the start of the plugin: the VFE posterior
    fit = vfe().fit(yd)
    lb = torch.tril(fit.lb[:m, :m])
    mu = torch.linalg.solve_triangular(lb.t(), fit.gamma, upper=True).t().contiguous()
    p = lb[None].contiguous()
    t_elbo, t_vfe = timed((lambda: svgp().elbo_grad(yd, mu, p), lambda: vfe().lml_grad(yd, want_z=False)), args.reps)
    # the entry points on the call's own operands
    blk = svgp()
    blk._enqueue_lu()
    a0 = blk.cov.cross(blk._xs, blk._zs)
    dev.trsm_rows(blk.lu, m, blk.ws_u, a0, n)
    pb, ws_p, _, gamma = blk._enqueue_column(mu[0], lb)
    w0 = a0.clone()
    dev.trsm_rows(pb, m, ws_p, w0, n)
    kdiag = blk._kdiag(blk._xs)
    nodes = torch.as_tensor(hermite_nodes()).to("cuda")
    outs = {k: torch.empty(n, dtype=tdt, device="cuda") for k in ("mean", "var", "g1", "g2")}
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    tail_mean, tail_var = torch.empty((n, 1), dtype=tdt, device="cuda"), torch.empty(n, dtype=tdt, device="cuda")
    rows = lambda lik: devs.svgp_rows(a0, w0, n, m, gamma, kdiag, yd[:, 0], nodes, lik, noise, 3.0, sums=sums, **outs)
    rows(1)
    g1, g2 = outs["g1"].clone(), outs["g2"].clone()
    scratch = torch.empty(dev.wsyrk_tn_scratch_bytes(n, m, 1, tdt), dtype=torch.uint8, device="cuda")
    c, g = dev.alloc_matrix(m, m, tdt, "cuda"), torch.empty((m, 1), dtype=tdt, device="cuda")
    t_rows_t, t_rows_g, t_tail, t_mom, t_wsyrk = timed((
        lambda: rows(1), lambda: rows(0),
        lambda: dev.sparse_tail(a0, w0, n, m, gamma[:, None], 1.0, 0.01, tail_mean, tail_var),
        lambda: devs.svgp_moments(a0, n, m, g2, g1[:, None], out=c, g=g, scratch=scratch),
        lambda: dev.wsyrk_tn(a0, n, m, g2, g1[:, None], 0.0, out=c, g=g, scratch=scratch)), args.reps)
    judged = m == 1000
    emit({"case": "svgp", "device": dev_name, "dtype": "f64", "n": n, "m": m, "d": d, "q": q, "nodes": 20,
          "svgp_rows_student_t_ms": t_rows_t, "svgp_rows_gaussian_ms": t_rows_g, "sparse_tail_ms": t_tail,
          "svgp_rows_over_sparse_tail": t_rows_t / t_tail, "svgp_moments_ms": t_mom, "wsyrk_tn_ms": t_wsyrk,
          "svgp_moments_over_wsyrk_tn": t_mom / t_wsyrk, "judged": judged,
          "within_1_10": bool(t_rows_t / t_tail <= 1.10 and t_mom / t_wsyrk <= 1.10) if judged else None,
          "elbo_grad_ms": t_elbo, "vfe_lml_grad_ms": t_vfe, "elbo_grad_over_vfe_lml_grad": t_elbo / t_vfe,
          "svgp_rows_bytes_per_s": 2 * 8.0 * n * m / (t_rows_t * 1e-3)})
    del blk, a0, w0, scratch, c, fit
    torch.cuda.empty_cache()
