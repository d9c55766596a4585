"""Timing of the gradient of the bound on uncertain inputs (include/cimrgp_psi_grad.h) on one GPU, by the method of
tools/bench_psi.py: FP64, device events after warm-up, median of --reps, the variants alternating in one process, at
(n, m) = (65536, 100) and (65536, 1000), d = 2, q = 1, per-row variances.  Three records per m:
  * kernels      cimrgp_psi2_grad and cimrgp_psi1_grad beside cimrgp_psi2 and cimrgp_psi1, and their ratios (two passes over
                 the n m^2 / 2 exponentials: about 2 is expected of psi2_grad / psi2);
  * gradient     one fit().bound_grad() (and bound_grad() alone) against the d + 3 fit().bound() evaluations that one
                 two-point gradient of L-BFGS-B costs, the latter on the ``BGPLVM`` path (``UncertainInputBlock.fit``);
  * optimise     the wall time of ``optimize=True`` for --iters L-BFGS-B iterations, ``BayesianGPLVM(jac='analytic')`` against
                 ``BGPLVM`` (two-point), and the bounds reached.
The figures are reported, with no threshold.  One JSON line per record on stdout, appended to the file named by the first
argument if given; ``runs`` says how many timed runs a median is of (the optimisations are timed once each)."""
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
from cimrgp_amd import device_psi as devp
from cimrgp_amd.GPLVM import BayesianGPLVM

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--m", type=int, nargs="*", default=[100, 1000])
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


d, q, n = 2, 1, 65536
for m in args.m:
    rng = np.random.default_rng(m)
    x = rng.normal(size=(n, d))
    y = (np.sin(2 * x).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    s = 10.0 ** rng.uniform(-3, -1, size=(n, d))
    xd, yd, sd = (dev.to_device(a, tdt, "cuda") for a in (x, y, s))
    zd = xd[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    ell = np.array([0.8, 1.2])
    block = lambda: ca.UncertainInputBlock(xd, sd, zd, ca.RBFKernel(l=1.0, sf=1.0, noise=0.1), 1e-6, lengthscales=ell)
    blk = block().fit(yd)
    ell_dev = blk._ell_dev
    common = dict(device=dev_name, dtype="f64", n=n, m=m, d=d, q=q, runs=args.reps, warmup=args.warmup)

    # ---- 1. the kernels ----
    gen = torch.Generator(device="cuda").manual_seed(m)
    g1 = torch.randn((n, dev.padded_ld(m)), generator=gen, dtype=tdt, device="cuda")
    g2 = torch.randn((m, m), generator=gen, dtype=tdt, device="cuda")
    g2 = (g2 + g2.t()).contiguous()
    out1, out2 = dev.alloc_matrix(n, m, tdt, xd.device), dev.alloc_matrix(m, m, tdt, xd.device)
    sc = {name: torch.empty(max(nb, 16), dtype=torch.uint8, device=xd.device)
          for name, nb in (("psi2", devp.psi2_scratch_bytes(n, m, d, tdt)), ("psi1g", devp.psi1_grad_scratch_bytes(n, m, d, tdt)),
                           ("psi2g", devp.psi2_grad_scratch_bytes(n, m, d, tdt)))}
    bad = torch.zeros(1, dtype=torch.float64, device=xd.device)
    o1 = [torch.empty((n, d), dtype=tdt, device="cuda"), torch.empty((n, d), dtype=tdt, device="cuda"),
          torch.empty((m, d), dtype=tdt, device="cuda"), torch.empty(d + 1, dtype=torch.float64, device="cuda")]
    o2 = [torch.empty_like(t) for t in o1]
    fns = (lambda: devp.psi2_grad(xd, sd, zd, ell_dev, 1.0, g2, *o2, scratch=sc["psi2g"], bad=bad),
           lambda: devp.psi1_grad(xd, sd, zd, ell_dev, 1.0, g1, *o1, scratch=sc["psi1g"]),
           lambda: devp.psi2(xd, sd, zd, ell_dev, 1.0, out=out2, scratch=sc["psi2"], bad=bad),
           lambda: devp.psi1(xd, sd, zd, ell_dev, 1.0, out=out1))
    t = timed(fns, args.reps, args.warmup)
    exps = n * m * (m + 1) // 2
    emit(dict(what="psi_grad kernels", psi2_grad_ms=t[0], psi1_grad_ms=t[1], psi2_ms=t[2], psi1_ms=t[3], psi2_grad_over_psi2=t[0] / t[2],
              psi1_grad_over_psi1=t[1] / t[3], psi2_grad_gexp_per_s=2 * exps / t[0] / 1e6, psi2_gexp_per_s=exps / t[2] / 1e6,
              psi2_grad_scratch_mib=round(sc["psi2g"].numel() / 2 ** 20, 1), psi1_grad_scratch_mib=round(sc["psi1g"].numel() / 2 ** 20, 1),
              **common))
    del g1, out1

    # ---- 2. one gradient evaluation ----
    def two_point():
        for _ in range(d + 3):
            block().fit(yd).bound()

    t = timed((lambda: block().fit(yd).bound_grad(), lambda: blk.bound_grad(), two_point, lambda: block().fit(yd).bound()), args.reps,
              args.warmup)
    emit(dict(what="psi_grad gradient", fit_and_bound_grad_ms=t[0], bound_grad_alone_ms=t[1], two_point_gradient_ms=t[2],
              two_point_evaluations=d + 3, fit_and_bound_ms=t[3], two_point_over_analytic=t[2] / t[0], **common))

    # ---- 3. a fixed number of L-BFGS-B iterations ----
    kw = dict(num_inducing=m, X_var=s, noise=0.1, optimize=True, max_iters=args.iters)

    def run(model):
        """(the fitted model or None, wall ms, the error's text or None): a two-point trial step may leave the kernel's domain."""
        try:
            _, ms = wall(lambda: model.fit([x, y]))
            return model, ms, None
        except ValueError as e:
            return None, float("nan"), str(e)

    for _ in range(2):                                                   # the first round warms both paths up
        analytic, ta, ea = run(BayesianGPLVM(jac='analytic', **kw))
        parent, tp, ep = run(ca.BGPLVM(**kw))
    start = ca.BGPLVM(num_inducing=m, X_var=s, noise=0.1)
    start.fit([x, y])
    reached = lambda g: None if g is None else g.block.bound()
    nfev = lambda g: None if g is None else int(g.optimizer_result.nfev)
    emit(dict(what="psi_grad optimise", iterations=args.iters, analytic_ms=ta, two_point_ms=tp, bound_start=start.block.bound(),
              bound_analytic=reached(analytic), bound_two_point=reached(parent), analytic_nfev=nfev(analytic), two_point_nfev=nfev(parent),
              analytic_error=ea, two_point_error=ep, **common))
