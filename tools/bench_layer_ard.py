"""One evaluation of a layer's hyper-parameter objective under ARD (cimrgp_layer_lml_grad_ard_cov: LML + d + 2 gradient
entries over all its blocks), device events after warm-up, median of ``--reps`` (5), at 128 x 2048, 64 x 4096 and 16 x 8192
(d = 2, q = 2, f64), against
  (a) cimrgp_layer_lml_grad_cov of the same run -- the two calls alternate, repetition by repetition, in one process -- and
  (b) the loop of the single-block ARD objective (RegressionInput.log_marginal_likelihood with a length-scale vector) over
      the same blocks, each on its residual targets: what the model would run without the batched call.
The ARD call runs on inputs divided by (l, l), so both calls factor the same matrices.  One JSON line per case on stdout,
appended to the file named by the first argument if given; ``--only BxN`` runs one shape, ``--cov`` one covariance.  The
commit is taken from CIMRGP_COMMIT (or git)."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cimrgp_amd import device as dev
from cimrgp_amd.Hyper import unit_lengthscale
from cimrgp_amd.RegressionInput import log_marginal_likelihood

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--only")
ap.add_argument("--cov", choices=("rbf", "matern32"))
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


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps, warmup=2):
    """Median milliseconds of every function of ``fns``, run in turn in each repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(event_ms(fn))
    return [float(np.median(t)) for t in ts]


SHAPES = [(128, 2048), (64, 4096), (16, 8192)]
if args.only:
    b, n = (int(v) for v in args.only.lower().split("x"))
    SHAPES = [(b, n)]
COVS = [("rbf", 0), ("matern32", 2)]
if args.cov:
    COVS = [c for c in COVS if c[0] == args.cov]
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
    out_ard = torch.empty((batch, d + 3), dtype=torch.float64, device="cuda")
    ell, sf2, nz = 0.3, 1.0, 0.05
    ells = np.full(d, ell)
    xs = unit_lengthscale(x, ells)[1]
    for name, cov in COVS:
        def iso():
            dev.layer_lml_grad(x, y, fbar, starts, n, ell, sf2, nz, None, karena, kinv, ws, info, out, cov=cov)

        def ard():
            dev.layer_lml_grad_ard(xs, y, fbar, starts, n, sf2, nz, None, karena, kinv, ws, info, out_ard, cov=cov)

        def loop():
            for b in range(batch):
                yb, fb = y[b * n:(b + 1) * n], fbar[b * n:(b + 1) * n]
                r = dev.residual(yb, fb, dev.block_stats(yb, fb)[:q])
                log_marginal_likelihood(x[b * n:(b + 1) * n], r, ells, sf2, nz, cov)

        t_iso, t_ard = alternating([iso, ard], args.reps)
        assert int(info.max().item()) == 0
        v_iso, v_ard = out.cpu().numpy(), out_ard.cpu().numpy()
        t_loop = alternating([loop], max(1, min(args.reps, 3)), warmup=1)[0]
        emit(dict(case="layer_lml_grad_ard", cov=name, batch=batch, n=n, d=d, q=q, dtype="f64",
                  ms=dict(ard=round(t_ard, 3), isotropic=round(t_iso, 3), single_block_ard_loop=round(t_loop, 3)),
                  ard_over_isotropic=round(t_ard / t_iso, 3), loop_over_ard=round(t_loop / t_ard, 2),
                  lml_sum=float(v_ard[:, 0].sum()), lml_sum_isotropic=float(v_iso[:, 0].sum())))
    del karena, kinv, ws
    torch.cuda.empty_cache()
