"""Timing of the greedy inducing-point selection (include/cimrgp_inducing.h) on one GPU, by the method of
tools/bench_psi_rows.py: FP64, device events after warm-up, median of --reps, at (n, m) = (65536, 1000), (65536, 100) and
(8192, 1000), d = 2, RBF.  Beside each time:
  * the traffic model n m^2 / 2 x 8 bytes (the reads of the earlier columns; the writes and the pivot-row gathers are O(n m))
    as bytes per second and as a fraction of the copy bandwidth this script measures on the same device (a 1 GiB
    device-to-device copy, read + write counted);
  * one ``SparseBlock.lml_grad`` evaluation at the same shape (random rows as Z): what a learned Z pays per objective
    evaluation, hundreds of times.
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
from cimrgp_amd import device_inducing as devi

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--shapes", type=int, nargs="*", default=[65536, 1000, 65536, 100, 8192, 1000], help="n m n m ..")
ap.add_argument("--no-lml-grad", action="store_true")
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


def timed(fn, reps, warmup):
    """Median time (ms) of the callable, device events around each call."""
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


# the copy bandwidth of this device: 1 GiB read and 1 GiB written per copy
src = torch.empty(1 << 27, dtype=tdt, device="cuda").normal_()
dst = torch.empty_like(src)
copy_ms = timed(lambda: dst.copy_(src), 7, 2)
copy_bw = 2 * src.numel() * 8 / (copy_ms * 1e-3)
del src, dst
emit(dict(what="copy bandwidth", device=dev_name, gib=1, copy_ms=copy_ms, copy_gb_per_s=copy_bw / 1e9))

d, ell = 2, 0.05
for n, m in zip(args.shapes[0::2], args.shapes[1::2]):
    rng = np.random.default_rng(n + m)
    x = rng.uniform(size=(n, d))
    y = np.sin(6 * x).sum(axis=1, keepdims=True) + 0.1 * rng.normal(size=(n, 1))
    xd, yd = dev.to_device(x, tdt, "cuda"), dev.to_device(y, tdt, "cuda")
    piv = torch.empty(m, dtype=torch.int64, device="cuda")
    lt = torch.empty((m, dev.padded_ld(n)), dtype=tdt, device="cuda")
    diag, trace = torch.empty(n, dtype=tdt, device="cuda"), torch.empty(m + 1, dtype=tdt, device="cuda")
    rank = torch.empty(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(max(devi.pivoted_cholesky_scratch_bytes(n, m), 16), dtype=torch.uint8, device="cuda")
    t = timed(lambda: devi.pivoted_cholesky(xd, m, ell, 1.0, pivots=piv, lt=lt, diag=diag, trace=trace, rank=rank, scratch=scratch),
              args.reps, args.warmup)
    tr = trace.cpu().numpy()
    model_bytes = n * m * m / 2 * 8
    rec = dict(what="pivoted cholesky", device=dev_name, dtype="f64", n=n, m=m, d=d, cov="rbf", ell=ell, runs=args.reps,
               warmup=args.warmup, pivoted_cholesky_ms=t, us_per_step=1e3 * t / m, model_gb=model_bytes / 1e9,
               model_gb_per_s=model_bytes / (t * 1e-3) / 1e9, fraction_of_copy_bandwidth=model_bytes / (t * 1e-3) / copy_bw,
               rank=int(rank.item()), trace_left=float(tr[m] / tr[0]))
    if not args.no_lml_grad:
        zd = xd[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
        blk = ca.SparseBlock(xd, zd, ca.RBFKernel(l=ell, sf=1.0, noise=0.01), 'vfe')
        g = timed(lambda: blk.lml_grad(yd), max(3, args.reps // 2), 1)
        rec.update(lml_grad_ms=g, pivoted_cholesky_over_lml_grad=t / g)
    emit(rec)
    del lt
