"""Timing of the psi statistics (include/cimrgp_psi.h) on one GPU: FP64, device events after warm-up, median of --reps, the
variants alternating in one process, at (n, m) = (65536, 100) and (65536, 1000), d = 2, q = 1, on ONE data set whose rows all
have the same variance vector (so that both routes compute the same Psi2):
  * cimrgp_psi2 on the (n, d) array of variances: the n m (m + 1) / 2 exponentials (with cimrgp_psi1 beside it);
  * the shared-variance route on the same data: two scalings, cimrgp_cov_cross, cimrgp_wsyrk_tn and the m x m factor;
  * cimrgp_wsyrk_tn alone on the n x m operand of that route;
  * one UncertainInputBlock.fit by each route.
The figures are reported, with no threshold: an exp-bound kernel and a matrix-core kernel have no common yardstick.  FP32
and several GPUs are not timed.  One JSON line per case on stdout, appended to the file named by the first argument if
given; ``runs`` says how many timed runs the median is of."""
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


d, q, n = 2, 1, 65536
for m in (100, 1000):
    rng = np.random.default_rng(m)
    x = rng.normal(size=(n, d))
    y = (np.sin(2 * x).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    svec = np.array([0.01, 0.04])
    xd, yd = dev.to_device(x, tdt, "cuda"), dev.to_device(y, tdt, "cuda")
    sd = dev.to_device(np.broadcast_to(svec, (n, d)), tdt, "cuda")
    zd = xd[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    ell = np.array([0.8, 1.2])
    kernel = lambda: ca.RBFKernel(l=1.0, sf=1.0, noise=0.1)
    rows = ca.UncertainInputBlock(xd, sd, zd, kernel(), 1e-6, lengthscales=ell)
    shared = ca.UncertainInputBlock(xd, svec, zd, kernel(), 1e-6, lengthscales=ell)
    ell_dev = rows._ell_dev
    out1, out2 = dev.alloc_matrix(n, m, tdt, xd.device), dev.alloc_matrix(m, m, tdt, xd.device)
    scratch = torch.empty(devp.psi2_scratch_bytes(n, m, d, tdt), dtype=torch.uint8, device=xd.device)
    bad = torch.zeros(1, dtype=torch.float64, device=xd.device)
    g = dev.rbf_cross(xd, zd, 1.0, 1.0)
    ones = torch.ones(n, dtype=tdt, device=xd.device)
    gout = dev.alloc_matrix(m, m, tdt, xd.device)
    gscratch = torch.empty(max(dev.wsyrk_tn_scratch_bytes(n, m, 0, tdt), 16), dtype=torch.uint8, device=xd.device)
    fns = (lambda: devp.psi2(xd, sd, zd, ell_dev, 1.0, out=out2, scratch=scratch, bad=bad),
           lambda: devp.psi1(xd, sd, zd, ell_dev, 1.0, out=out1),
           lambda: shared._psi2(),
           lambda: dev.wsyrk_tn(g, n, m, ones, out=gout, scratch=gscratch),
           lambda: ca.UncertainInputBlock(xd, sd, zd, kernel(), 1e-6, lengthscales=ell).fit(yd),
           lambda: ca.UncertainInputBlock(xd, svec, zd, kernel(), 1e-6, lengthscales=ell).fit(yd))
    t = timed(fns, args.reps, args.warmup)
    # the two routes computed the same matrix
    p_rows, p_shared = devp.psi2(xd, sd, zd, ell_dev, 1.0)[0], shared._psi2()[0]
    low = torch.tril(torch.ones((m, m), dtype=torch.bool, device=xd.device))
    diff = float(((p_rows[:m, :m] - p_shared[:m, :m]).abs()[low] / p_shared[:m, :m].abs()[low].clamp_min(1e-300)).max().item())
    exps = n * m * (m + 1) // 2
    emit(dict(what="psi", device=dev_name, dtype="f64", n=n, m=m, d=d, q=q, runs=args.reps, warmup=args.warmup,
              slices=devp.psi2_slices(n, m), scratch_mib=round(scratch.numel() / 2 ** 20, 1),
              psi2_ms=t[0], psi2_gexp_per_s=exps / t[0] / 1e6, psi1_ms=t[1], shared_route_psi2_ms=t[2], wsyrk_tn_ms=t[3],
              fit_rows_ms=t[4], fit_shared_ms=t[5], routes_max_rel_diff=diff, bound_rows=rows.fit(yd).bound(),
              bound_shared=shared.fit(yd).bound()))
