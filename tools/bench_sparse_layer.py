"""Timing of sparse (inducing-point) layers in the multiresolution model ("Sparse layers in the multiresolution
model") on one GPU, FP64: the chain of config 3 (workloads.make_chain_1d: N = 65536, d = 1, q = 2, IndexSetUniform(N, 4, 2) =
five layers of 1 .. 16 regions, N / 4 test points, RBF with l_j = 2^-j, sf = 1, noise 0.01) all exact against the same chain
with layers 0 - 2 sparse (FITC, m = 1024, inducing rows by stride).  The two variants alternate in one process; wall time
after one warm-up round, median of --reps: fit() and get_predicted_mean_and_var; with them layer_fit_ms() per layer (device
events of the last repetition), the peak device memory of fit + prediction, and the standardised mean squared error of both
variants at the test points against the noise-free targets -- REPORTED, not judged: the sparse model is an approximation and
how good it is depends on the data.  FP32, several GPUs and N beyond 65536 are not timed.  One JSON line on stdout, appended
to the file named by the first argument if given."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
import workloads
from cimrgp_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--m", type=int, default=1024)
ap.add_argument("--sparse-layers", type=int, default=3, help="layers 0 .. this - 1 are sparse in the sparse variant")
args = ap.parse_args()
dev.require_gpu()

n, q, res = args.n, 2, 4
x, y, xs = workloads.make_chain_1d(n, q)
ns = xs.shape[0]
truth = workloads.targets_1d(xs, q, np.random.default_rng(0), noise_sd=0.0)
ells = workloads.chain_length_scales(res + 1, 1)
idx, idx_t = ca.IndexSetUniform(n, res, 2), ca.IndexSetUniform(ns, res, 2)
exact = [ca.RBFKernel(l=l, sf=1.0, noise=0.01) for l in ells]
sparse = [ca.SparseKernel(k, num_inducing=args.m, approximation='fitc', inducing='stride') if j < args.sparse_layers else k
          for j, k in enumerate(exact)]
VARIANTS = (("exact", exact), ("sparse", sparse))


def one_round(kernels):
    """fit + predict of one variant: (fit wall ms, predict wall ms, per-layer device ms, peak bytes, smse)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=idx, spectral_density_obj=kernels)
    model.fit()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mean, var = model.get_predicted_mean_and_var(xs, idx_t)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    layer_ms = model.layer_fit_ms()
    peak = torch.cuda.max_memory_allocated() - base
    del model
    smse = float(np.mean(((mean - truth) ** 2).mean(axis=0) / truth.var(axis=0)))
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), layer_ms, peak, smse


for _, kernels in VARIANTS:                                 # warm-up: the streams, the look-ahead contexts, the allocator
    one_round(kernels)
runs = {name: [] for name, _ in VARIANTS}
for _ in range(args.reps):
    for name, kernels in VARIANTS:
        runs[name].append(one_round(kernels))

rec = {"case": "sparse_layers_config3_chain", "device": torch.cuda.get_device_name(0), "dtype": "f64", "n": n, "n_test": ns, "d": 1,
       "q": q, "layers": res + 1, "regions": [len(b) for b in idx.bounds], "reps": args.reps, "m": args.m,
       "sparse_layers": list(range(args.sparse_layers)), "approximation": "fitc", "inducing": "stride"}
for name, _ in VARIANTS:
    r = runs[name]
    rec[name] = {"fit_wall_ms": float(np.median([v[0] for v in r])),
                 "predict_mean_and_var_wall_ms": float(np.median([v[1] for v in r])),
                 "layer_fit_ms": [float(v) for v in r[-1][2]],
                 "peak_device_mib": max(v[3] for v in r) / 2.0 ** 20,
                 "smse": r[-1][4]}
rec["fit_exact_over_sparse"] = rec["exact"]["fit_wall_ms"] / rec["sparse"]["fit_wall_ms"]
rec["predict_exact_over_sparse"] = rec["exact"]["predict_mean_and_var_wall_ms"] / rec["sparse"]["predict_mean_and_var_wall_ms"]
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
# the one condition: the sparse variant's fit is faster than the all-exact fit of the same run
if not rec["sparse"]["fit_wall_ms"] < rec["exact"]["fit_wall_ms"]:
    sys.exit("the sparse variant's fit (%.1f ms) is not faster than the all-exact fit (%.1f ms)"
             % (rec["sparse"]["fit_wall_ms"], rec["exact"]["fit_wall_ms"]))
