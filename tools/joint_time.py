"""The joint-distribution calls of one layer (include/cimrgp_joint.h), CUDA events after warm-up, at the layer shapes
of profiles/layer_lml_times.jsonl -- 128 x 2048, 64 x 4096, 16 x 8192 (d = 2, q = 2, f64, RBF) -- with ns = n / 4
test points per block and size in {8, 256} samples (cols = size q sample columns):
  * cimrgp_layer_predict (mean and variance, for scale),
  * cimrgp_layer_joint_cov with the factor,
  * cimrgp_normal_fill and cimrgp_layer_sample at each size,
and the sample kernel's rate: sum_b ns (ns + 1) / 2 cols 2 flop over its time, as a share of the 78.6 TF/s FP64
matrix peak.  One JSON line per case on stdout, appended to the file named by the first argument if given; ``--only
BxN`` runs one shape, ``--reps R`` sets the repetitions.  The kernel breakdown comes from a separate rocprofv3
--kernel-trace --stats run."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cimrgp_amd import device as dev
from cimrgp_amd.Posteriors import NOISE_FLOOR, NOISE_FRACTION

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--only")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev.require_gpu()
PEAK_F64 = 78.6e12


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
    ns = n // 4
    big = batch * n
    x = dev.to_device(np.sort(rng.uniform(-1.7, 1.7, size=(big, d)), axis=0), dt, "cuda")
    y = dev.to_device(rng.normal(size=(big, q)), dt, "cuda")
    xs = dev.to_device(np.sort(rng.uniform(-1.7, 1.7, size=(batch * ns, d)), axis=0), dt, "cuda")
    starts = torch.arange(batch, dtype=torch.int64, device="cuda") * n
    t_starts = torch.arange(batch, dtype=torch.int64, device="cuda") * ns
    ld = dev.padded_ld(n)
    ws_bytes = max((dev.potrf_workspace_bytes(n, dt) + 15) // 16 * 16, 16)
    karena = torch.empty((batch, n, ld), dtype=dt, device="cuda")
    ws = torch.empty((batch, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    bias = torch.empty((batch, q), dtype=dt, device="cuda")
    noise = torch.empty(batch, dtype=dt, device="cuda")
    z = torch.empty((batch, n, q), dtype=dt, device="cuda")
    alpha = torch.empty((batch, n, q), dtype=dt, device="cuda")
    ell, sf2, nz = 0.3, 1.0, 0.05
    dev.layer_fit(x, y, None, torch.zeros_like(y), starts, n, ell, sf2, nz, NOISE_FRACTION, NOISE_FLOOR, None, None, karena, ws, info,
                  bias, noise, z, alpha)
    assert int(info.max().item()) == 0
    mean = torch.zeros((batch * ns, q), dtype=dt, device="cuda")
    var = torch.zeros(batch * ns, dtype=dt, device="cuda")
    ldc = dev.padded_ld(ns)
    carena = torch.empty((batch, ns, ldc), dtype=dt, device="cuda")
    cws = torch.empty((batch, max((dev.potrf_workspace_bytes(ns, dt) + 15) // 16 * 16, 16)), dtype=torch.uint8, device="cuda")
    cinfo = torch.zeros(batch, dtype=torch.int32, device="cuda")
    diag = torch.full((batch,), 1e-6 * sf2, dtype=dt, device="cuda") + noise

    def predict():
        dev.layer_predict(x, starts, n, xs, t_starts, ns, ell, sf2, karena, ws, z, bias, noise, mean, var)

    def joint():
        dev.layer_joint_cov(x, starts, n, xs, t_starts, ns, ell, sf2, karena, ws, diag, carena, cws, cinfo)

    t_p = timed(predict, args.reps)
    t_j = timed(joint, args.reps)
    assert int(cinfo.abs().max().item()) == 0
    keys = torch.arange(batch, dtype=torch.int64, device="cuda")
    for size in (8, 256):
        cols = size * q
        zbuf = torch.empty((batch, cols, ldc), dtype=dt, device="cuda")
        out = torch.zeros((cols, batch * ns), dtype=dt, device="cuda")

        def fill():
            dev.normal_fill(0, keys, 0, cols, ns, zbuf)

        def sample():
            dev.layer_sample(carena, ns, zbuf, cols, t_starts, out)

        t_n = timed(fill, args.reps)
        t_s = timed(sample, args.reps)
        flops = batch * ns * (ns + 1) / 2 * cols * 2
        emit(dict(case="joint", cov="rbf", batch=batch, n=n, ns=ns, size=size, cols=cols, d=d, q=q, dtype="f64",
                  ms=dict(layer_predict=round(t_p, 3), layer_joint_cov=round(t_j, 3), normal_fill=round(t_n, 3),
                          layer_sample=round(t_s, 3)),
                  joint_cov_over_predict=round(t_j / t_p, 3), sample_tflops=round(flops / (t_s * 1e-3) / 1e12, 2),
                  sample_share_of_f64_peak=round(flops / (t_s * 1e-3) / PEAK_F64, 3)))
        del zbuf, out
    del karena, ws, carena, cws, z, alpha
    torch.cuda.empty_cache()
