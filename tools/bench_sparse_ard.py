"""Timing of the ARD length-scales of the sparse GP (include/cimrgp_sparse_ard.h) on one GPU: FP64, device events after
warm-up, median of --reps, the variants alternating in one process, at (n, m) = (65536, 1024), q = 1, d = 2 and d = 8, RBF,
FITC:
  * cimrgp_cov_pair_grad_ard against its twin cimrgp_cov_pair_grad on the same operands (the ratio is reported, not judged);
  * SparseBlock.lml_grad with lengthscales (d + 2 + m d derivatives) against the isotropic lml_grad (3 + m d);
  * one evaluation of the objective (fit + log_marginal_likelihood) with lengthscales.
The one condition: the time ARD adds to a gradient call (lml_grad with lengthscales minus isotropic lml_grad) is less than
d evaluations, what two-point differences over d length-scales would spend instead ("added_below_d_evaluations").
One JSON line per d on stdout, appended to the file named by the first argument if given."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cimrgp_amd import device as dev
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


def timed(fns, reps, warmup=2):
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
    return [float(np.median(t)) for t in ts]


n, m, q = 65536, 1024, 1
for d in (2, 8):
    rng = np.random.default_rng(n + d)
    xh = rng.uniform(-2, 2, size=(n, d))
    yh = (np.sin(2 * xh).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
    x, y = dev.to_device(xh, tdt, "cuda"), dev.to_device(yh, tdt, "cuda")
    z = x[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
    # equal length-scales 0.4 sqrt(d): both blocks evaluate the same covariance (the same exponentials, the same conditioning)
    ell = 0.4 * np.sqrt(d)
    noise = 0.01
    ard_block = lambda: SparseBlock(x, z, RBFKernel(l=1.0, sf=1.0, noise=noise), 'fitc', 1e-6, lengthscales=np.full(d, ell))
    iso_block = lambda: SparseBlock(x, z, RBFKernel(l=ell, sf=1.0, noise=noise), 'fitc', 1e-6)
    t_ard, t_iso, t_eval_ard, t_eval_iso = timed((lambda: ard_block().lml_grad(y), lambda: iso_block().lml_grad(y),
                                                  lambda: ard_block().fit(y).log_marginal_likelihood(),
                                                  lambda: iso_block().fit(y).log_marginal_likelihood()), args.reps)
    # the two contractions on the same operands: a weight matrix of the size and pitch of G_fu
    gbuf = dev.alloc_matrix(n, m, tdt, "cuda")
    gbuf.normal_()
    xs, zs = (x / ell).contiguous(), (z / ell).contiguous()
    scr_t = torch.empty(dev.cov_pair_grad_scratch_bytes(n, m, d), dtype=torch.uint8, device="cuda")
    scr_a = torch.empty(dev.cov_pair_grad_ard_scratch_bytes(n, m, d), dtype=torch.uint8, device="cuda")
    s_t, s_a = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1 + d, dtype=torch.float64, device="cuda")
    db_t, db_a = torch.zeros((m, d), dtype=tdt, device="cuda"), torch.zeros((m, d), dtype=tdt, device="cuda")
    t_pair_ard, t_pair_twin = timed((
        lambda: dev.cov_pair_grad_ard(xs, zs, gbuf, 1.0, 1.0, sums=s_a, db=db_a, scratch=scr_a),
        lambda: dev.cov_pair_grad(xs, zs, gbuf, 1.0, 1.0, sums=s_t, db=db_t, scratch=scr_t)), args.reps)
    added = t_ard - t_iso
    emit({"case": "sparse_ard", "device": dev_name, "dtype": "f64", "approximation": "fitc", "cov": "rbf", "n": n, "m": m, "d": d,
          "q": q, "cov_pair_grad_ard_ms": t_pair_ard, "cov_pair_grad_ms": t_pair_twin,
          "cov_pair_grad_ard_over_twin": t_pair_ard / t_pair_twin, "lml_grad_ard_ms": t_ard, "lml_grad_isotropic_ms": t_iso,
          "evaluation_ard_ms": t_eval_ard, "evaluation_isotropic_ms": t_eval_iso, "added_by_ard_ms": added,
          "d_evaluations_ms": d * t_eval_ard, "added_below_d_evaluations": bool(added < d * t_eval_ard),
          "same_sum_k_and_db_bits": bool(torch.equal(s_a[:1].view(torch.int64), s_t[:1].view(torch.int64))
                                         and torch.equal(db_a.view(torch.int64), db_t.view(torch.int64)))})
    del x, y, z, gbuf, xs, zs, scr_t, scr_a
    torch.cuda.empty_cache()
