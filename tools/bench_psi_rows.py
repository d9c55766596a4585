"""Timing of the predictive variance at uncertain test inputs (include/cimrgp_psi_rows.h) on one GPU, by the method of
tools/bench_psi_grad.py: FP64, device events after warm-up, median of --reps, the variants alternating in one process, at
(ns, m) = (65536, 1000), d = 2, q = 1, per-row variances.  Two records per m:
  * kernel       cimrgp_psi2_rows_quad beside cimrgp_psi2 at the same (n, m, d): both pay n m (m + 1) / 2 exponentials, the
                 first per row against two weights, the second summed over the rows;
  * prediction   ``UncertainInputBlock.predict_moments`` (mean and variance) beside ``predict(xs_var=)`` (the mean alone)
                 and ``SparseBlock.predict`` at exact inputs (mean and variance).
The figures are reported, with no threshold.  One JSON line per record on stdout, appended to the file named by the first
argument if given; ``runs`` says how many timed runs a median is of."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
from cimrgp_amd import device as dev
from cimrgp_amd import device_psi as devp

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--m", type=int, nargs="*", default=[1000])
ap.add_argument("--q", type=int, default=1)
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


def timed(fns, reps, warmup):
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


d, q, n = 2, args.q, args.n
for m in args.m:
    rng = np.random.default_rng(m)
    x = rng.normal(size=(n, d))
    y = np.stack([np.sin((2 + c) * x).sum(axis=1) + 0.1 * rng.normal(size=n) for c in range(q)], axis=1)
    s = 10.0 ** rng.uniform(-3, -1, size=(n, d))
    xd, yd, sd = (dev.to_device(a, tdt, "cuda") for a in (x, y, s))
    zd = xd[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    ell = np.array([0.8, 1.2])
    blk = ca.UncertainInputBlock(xd, sd, zd, ca.RBFKernel(l=1.0, sf=1.0, noise=0.1), 1e-6, lengthscales=ell).fit(yd)
    ell_dev = blk._ell_dev
    common = dict(device=dev_name, dtype="f64", n=n, m=m, d=d, q=q, runs=args.reps, warmup=args.warmup)

    # ---- 1. the kernel beside cimrgp_psi2 ----
    gen = torch.Generator(device="cuda").manual_seed(m)
    c = torch.randn((m, m), generator=gen, dtype=tdt, device="cuda")
    c = (c + c.t()).contiguous()
    a = torch.randn((m, q), generator=gen, dtype=tdt, device="cuda")
    out2 = dev.alloc_matrix(m, m, tdt, xd.device)
    sc2 = torch.empty(max(devp.psi2_scratch_bytes(n, m, d, tdt), 16), dtype=torch.uint8, device=xd.device)
    scr = torch.empty(max(devp.psi2_rows_quad_scratch_bytes(n, m, d, q, tdt), 16), dtype=torch.uint8, device=xd.device)
    bad = torch.zeros(1, dtype=torch.float64, device=xd.device)
    tr, quad = torch.empty(n, dtype=tdt, device="cuda"), torch.empty((n, q), dtype=tdt, device="cuda")
    fns = (lambda: devp.psi2_rows_quad(xd, sd, zd, ell_dev, 1.0, c, a, tr=tr, quad=quad, scratch=scr, bad=bad),
           lambda: devp.psi2(xd, sd, zd, ell_dev, 1.0, out=out2, scratch=sc2, bad=bad))
    t = timed(fns, args.reps, args.warmup)
    exps = n * m * (m + 1) // 2
    emit(dict(what="psi_rows kernel", psi2_rows_quad_ms=t[0], psi2_ms=t[1], psi2_rows_quad_over_psi2=t[0] / t[1],
              psi2_rows_quad_gexp_per_s=exps / t[0] / 1e6, psi2_gexp_per_s=exps / t[1] / 1e6,
              psi2_rows_quad_scratch_mib=round(scr.numel() / 2 ** 20, 1), **common))
    del c, a, out2, sc2, scr

    # ---- 2. the prediction ----
    mean, var = torch.empty((n, q), dtype=tdt, device="cuda"), torch.empty((n, q), dtype=tdt, device="cuda")
    var1 = torch.empty(n, dtype=tdt, device="cuda")
    fns = (lambda: blk.predict_moments(xd, sd, mean, var), lambda: blk.predict(xd, mean, None, xs_var=sd),
           lambda: blk.predict(xd, mean, var1))
    t = timed(fns, args.reps, args.warmup)
    emit(dict(what="psi_rows prediction", predict_moments_ms=t[0], predict_mean_uncertain_ms=t[1], predict_exact_ms=t[2],
              moments_over_mean=t[0] / t[1], **common))
