"""One evaluation of a layer's hyper-parameter objective (LML + gradient over all its blocks), CUDA events after
warm-up, at 128 x 2048, 64 x 4096 and 16 x 8192 (d = 2, q = 2, f64; RBF and Matern 3/2), against
  * cimrgp_layer_fit at the same shape (the layer's fit, for scale), and
  * the loop of the single-block composition (RegressionInput.log_marginal_likelihood) over the same blocks, each on
    its residual targets -- what the model would run without the batched call.
One JSON line per case on stdout, appended to the file named by the first argument if given; ``--only BxN`` runs one
shape, ``--reps R`` sets the repetitions.  The commit is taken from CIMRGP_COMMIT (or git).  The kernel breakdown of
the batched call comes from a separate rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cimrgp_amd import device as dev
from cimrgp_amd.Posteriors import NOISE_FLOOR, NOISE_FRACTION
from cimrgp_amd.RegressionInput import log_marginal_likelihood

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--only")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()


def commit():
    c = os.environ.get("CIMRGP_COMMIT")
    if c:
        return c
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


COMMIT = commit()


def emit(rec):
    rec["commit"] = COMMIT
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


SHAPES = [(128, 2048), (64, 4096), (16, 8192)]
if args.only:
    b, n = (int(v) for v in args.only.lower().split("x"))
    SHAPES = [(b, n)]
d, q, dt = 2, 2, torch.float64
rng = np.random.default_rng(0)
for batch, n in SHAPES:
    big = batch * n
    x = dev.to_device(np.sort(rng.uniform(-1.7, 1.7, size=(big, d)), axis=0), dt, "cuda")
    y = dev.to_device(rng.normal(size=(big, q)), dt, "cuda")
    fbar = torch.zeros_like(y)
    starts = torch.arange(batch, dtype=torch.int64, device="cuda") * n
    ld = dev.padded_ld(n)
    ws_bytes = max((dev.potrf_workspace_bytes(n, dt) + 15) // 16 * 16, 16)
    karena = torch.empty((batch, n, ld), dtype=dt, device="cuda")
    kinv = torch.empty((batch, n, ld), dtype=dt, device="cuda")
    ws = torch.empty((batch, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    out = torch.empty((batch, 4), dtype=torch.float64, device="cuda")
    bias = torch.empty((batch, q), dtype=dt, device="cuda")
    noise = torch.empty(batch, dtype=dt, device="cuda")
    z = torch.empty((batch, n, q), dtype=dt, device="cuda")
    alpha = torch.empty((batch, n, q), dtype=dt, device="cuda")
    train = torch.zeros_like(y)
    ell, sf2, nz = 0.3, 1.0, 0.05
    for name, cov in (("rbf", 0), ("matern32", 2)):
        def batched():
            dev.layer_lml_grad(x, y, fbar, starts, n, ell, sf2, nz, None, karena, kinv, ws, info, out, cov=cov)

        def fit():
            dev.layer_fit(x, y, fbar, train, starts, n, ell, sf2, nz, NOISE_FRACTION, NOISE_FLOOR, None, None, karena, ws, info,
                          bias, noise, z, alpha, cov=cov)

        def loop():
            for b in range(batch):
                yb, fb = y[b * n:(b + 1) * n], fbar[b * n:(b + 1) * n]
                r = dev.residual(yb, fb, dev.block_stats(yb, fb)[:q])
                log_marginal_likelihood(x[b * n:(b + 1) * n], r, ell, sf2, nz, cov)

        t_b = timed(batched, args.reps)
        assert int(info.max().item()) == 0
        vals = out.cpu().numpy()
        t_f = timed(fit, args.reps)
        t_l = timed(loop, max(1, min(args.reps, 3)), warmup=1)
        emit(dict(case="layer_lml_grad", cov=name, batch=batch, n=n, d=d, q=q, dtype="f64",
                  ms=dict(batched=round(t_b, 3), layer_fit=round(t_f, 3), single_block_loop=round(t_l, 3)),
                  batched_over_layer_fit=round(t_b / t_f, 3), loop_over_batched=round(t_l / t_b, 2),
                  lml_sum=float(vals[:, 0].sum())))
    del karena, kinv, ws, z, alpha
    torch.cuda.empty_cache()
