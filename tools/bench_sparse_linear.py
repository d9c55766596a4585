"""Timing of the sparse GP's linear term (include/cimrgp_sparse_linear.h) on one GPU: FP64, device events after warm-up,
median of --reps, the variants alternating in one process, at (n, m) = (65536, 1000), q = 1, d = 2 and d = 8, RBF with ARD
length-scales, VFE (the reference plugin's kernel and bound):
  * cimrgp_cov_cross_lin against cimrgp_cov_cross on the same operands (the ratio is reported, not judged);
  * cimrgp_cov_pair_grad_lin (ard) against cimrgp_cov_pair_grad_ard on the same operands (reported, not judged);
  * SparseBlock.lml_grad with and without ``linear``;
  * one evaluation of the objective (fit + log_marginal_likelihood) with ``linear``.
The one condition: the time the term adds to a gradient call (lml_grad with linear minus lml_grad without) is less than d
evaluations of the same run, what two-point differences over the d new parameters would spend instead
("added_below_d_evaluations").  The ``*_spread_ms`` fields are max - min over the repetitions of the four block-level times:
what a comparison of two runs' medians can tell apart.  One JSON line per d on stdout, appended to the file named by the
first argument if given."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cimrgp_amd import device as dev
from cimrgp_amd import device_linear as devl
from cimrgp_amd.KernelClass import RBFKernel
from cimrgp_amd.Sparse import SparseBlock

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


def timed(fns, reps, warmup=2, spread=None):
    """Median times (ms) of the callables, alternating, device events around each call (a call that reads back ends inside
    its events)."""
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


n, m, q = 65536, 1000, 1
for d in (2, 8):
    rng = np.random.default_rng(n + d)
    xh = rng.uniform(-2, 2, size=(n, d))
    yh = (np.sin(2 * xh).sum(axis=1) + 0.7 * xh[:, 0] + 0.1 * rng.normal(size=n))[:, None]
    x, y = dev.to_device(xh, tdt, "cuda"), dev.to_device(yh, tdt, "cuda")
    z = x[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    ells = np.full(d, 0.4 * np.sqrt(d))
    v = np.full(d, 0.3)
    noise = 0.01
    lin_block = lambda: SparseBlock(x, z, RBFKernel(l=1.0, sf=1.0, noise=noise), 'vfe', 1e-6, lengthscales=ells, linear=v)
    cov_block = lambda: SparseBlock(x, z, RBFKernel(l=1.0, sf=1.0, noise=noise), 'vfe', 1e-6, lengthscales=ells)
    spread = []
    t_lin, t_cov, t_eval_lin, t_eval_cov = timed((lambda: lin_block().lml_grad(y), lambda: cov_block().lml_grad(y),
                                                  lambda: lin_block().fit(y).log_marginal_likelihood(),
                                                  lambda: cov_block().fit(y).log_marginal_likelihood()), args.reps, spread=spread)
    # the kernels on the same operands: the scaled inputs, an output / a weight matrix of the size and pitch of K_fu / G_fu
    xs, zs = (x / torch.as_tensor(ells).to("cuda")).contiguous(), (z / torch.as_tensor(ells).to("cuda")).contiguous()
    lin = torch.as_tensor(v * ells ** 2).to("cuda")
    kbuf = dev.alloc_matrix(n, m, tdt, "cuda")
    t_cross_lin, t_cross = timed((lambda: devl.cov_cross_lin(xs, zs, 1.0, 1.0, lin, out=kbuf),
                                  lambda: dev.rbf_cross(xs, zs, 1.0, 1.0, out=kbuf)), args.reps)
    gbuf = kbuf
    gbuf.normal_()
    scr_l = torch.empty(devl.cov_pair_grad_lin_scratch_bytes(n, m, d, True), dtype=torch.uint8, device="cuda")
    scr_a = torch.empty(dev.cov_pair_grad_ard_scratch_bytes(n, m, d), dtype=torch.uint8, device="cuda")
    s_l, s_a = torch.zeros(1 + d, dtype=torch.float64, device="cuda"), torch.zeros(1 + d, dtype=torch.float64, device="cuda")
    ls = torch.zeros(d, dtype=torch.float64, device="cuda")
    db_l, db_a = torch.zeros((m, d), dtype=tdt, device="cuda"), torch.zeros((m, d), dtype=tdt, device="cuda")
    t_pair_lin, t_pair_ard = timed((
        lambda: devl.cov_pair_grad_lin(xs, zs, gbuf, 1.0, 1.0, lin, ard=True, sums=s_l, lsums=ls, db=db_l, scratch=scr_l),
        lambda: dev.cov_pair_grad_ard(xs, zs, gbuf, 1.0, 1.0, sums=s_a, db=db_a, scratch=scr_a)), args.reps)
    added = t_lin - t_cov
    emit({"case": "sparse_linear", "device": dev_name, "dtype": "f64", "approximation": "vfe", "cov": "rbf", "ard": True, "n": n, "m": m,
          "d": d, "q": q, "cov_cross_lin_ms": t_cross_lin, "cov_cross_ms": t_cross, "cov_cross_lin_over_twin": t_cross_lin / t_cross,
          "cov_pair_grad_lin_ms": t_pair_lin, "cov_pair_grad_ard_ms": t_pair_ard, "cov_pair_grad_lin_over_twin": t_pair_lin / t_pair_ard,
          "lml_grad_linear_ms": t_lin, "lml_grad_ms": t_cov, "evaluation_linear_ms": t_eval_lin, "evaluation_ms": t_eval_cov,
          "lml_grad_linear_spread_ms": spread[0], "lml_grad_spread_ms": spread[1], "evaluation_linear_spread_ms": spread[2],
          "evaluation_spread_ms": spread[3],
          "added_by_linear_ms": added, "d_evaluations_ms": d * t_eval_lin, "added_below_d_evaluations": bool(added < d * t_eval_lin),
          "same_sums_bits": bool(torch.equal(s_l.view(torch.int64), s_a.view(torch.int64)))})
    del x, y, z, kbuf, gbuf, xs, zs, scr_l, scr_a
    torch.cuda.empty_cache()
