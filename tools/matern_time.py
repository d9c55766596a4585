"""Matern covariances against the RBF in the same process, alternating, CUDA events after warm-up:
  * the f64 lower Gram (k_gram_lower_wide) at n = 8192 and 16384, d = 1 and 2
  * cimrgp_layer_fit[_cov] at 64 x 4096 and 128 x 2048 (d = 2, q = 2)
  * one GP_RBF / GP_Matern objective evaluation (LML + gradient: Gram, factorisation, K^-1, gradient) at n = 3000
One JSON line per case (median milliseconds per covariance and the ratio to the RBF) on stdout, and appended
to the file named by the first argument if given.  Run the kernel breakdown separately under
rocprofv3 --kernel-trace --stats."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cimrgp_amd as ca
from cimrgp_amd import device as dev

COVS = [("rbf", 0), ("matern12", 1), ("matern32", 2), ("matern52", 3)]
out_path = sys.argv[1] if len(sys.argv) > 1 else None
dev.require_gpu()
rng = np.random.default_rng(0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def alternate(fns, reps, warmup=3):
    """fns: name -> callable enqueueing the work; the names take turns inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ts.items()}


def ratios(ms):
    return {k: round(v / ms["rbf"], 3) for k, v in ms.items() if k != "rbf"}


# ---- lower Gram, f64 --------------------------------------------------------------------------------------
for n in (8192, 16384):
    k = dev.alloc_matrix(n, n, torch.float64, "cuda")
    for d in (1, 2):
        x = dev.to_device(rng.uniform(-1.7, 1.7, size=(n, d)), torch.float64, "cuda")
        fns = {name: (lambda c=c: dev.rbf_gram(x, 0.3, 1.0, 0.01, lower_only=True, out=k, cov=c)) for name, c in COVS}
        ms = alternate(fns, reps=30)
        us = {name: round(v * 1e3, 1) for name, v in ms.items()}
        emit(dict(case="gram_lower_f64", n=n, d=d, us=us, ratio_to_rbf=ratios(ms),
                  rbf_write_TBps=round(n * (n + 1) / 2 * 8 / (ms["rbf"] * 1e-3) / 1e12, 2)))
    del k
    torch.cuda.empty_cache()

# ---- layer_fit ---------------------------------------------------------------------------------------------
for nb, n in ((64, 4096), (128, 2048)):
    d, q = 2, 2
    x = torch.as_tensor(np.sort(rng.uniform(-1.7, 1.7, size=(nb * n, d)), axis=0)).cuda()
    y = torch.as_tensor(rng.normal(size=(nb * n, q))).cuda()
    starts = torch.arange(nb, dtype=torch.int64, device="cuda") * n
    ld = dev.padded_ld(n)
    karena = torch.empty((nb, n, ld), dtype=torch.float64, device="cuda")
    wsb = max((dev.potrf_workspace_bytes(n, torch.float64) + 15) // 16 * 16, 16)
    ws = torch.empty((nb, wsb), dtype=torch.uint8, device="cuda")
    info = torch.zeros(nb, dtype=torch.int32, device="cuda")
    bias = torch.empty((nb, q), dtype=torch.float64, device="cuda")
    noise = torch.empty(nb, dtype=torch.float64, device="cuda")
    z = torch.empty((nb, n, q), dtype=torch.float64, device="cuda")
    alpha = torch.empty((nb, n, q), dtype=torch.float64, device="cuda")
    tout = torch.zeros_like(y)

    def fit(c):
        dev.layer_fit(x, y, None, tout, starts, n, 0.3, 1.0, 0.01, 0.01, 1e-8, None, None, karena, ws, info, bias, noise,
                      z, alpha, cov=c)
    ms = alternate({name: (lambda c=c: fit(c)) for name, c in COVS}, reps=7, warmup=2)
    emit(dict(case="layer_fit_f64", nb=nb, n=n, d=d, q=q, ms={k: round(v, 3) for k, v in ms.items()}, ratio_to_rbf=ratios(ms),
              info_max=int(info.abs().max().item())))
    del karena, ws, x, y, z, alpha, tout
    torch.cuda.empty_cache()

# ---- one plugin objective evaluation -------------------------------------------------------------------------
n = 3000
x = dev.to_device(rng.uniform(-1.7, 1.7, size=(n, 2)), torch.float64, "cuda")
y = dev.to_device(np.sin(3 * x.cpu().numpy()) + 0.1 * rng.normal(size=(n, 2)), torch.float64, "cuda")
plugins = {"rbf": ca.GP_RBF(optimize=False)}
plugins.update({name: ca.GP_Matern(nu=nu, optimize=False) for name, nu in (("matern12", 0.5), ("matern32", 1.5),
                                                                               ("matern52", 2.5))})
ms = alternate({name: (lambda p=p: p.log_marginal_likelihood(x, y, 0.5, 1.0, 0.01)) for name, p in plugins.items()},
               reps=7, warmup=2)
emit(dict(case="gp_objective_f64", n=n, d=2, q=2, ms={k: round(v, 3) for k, v in ms.items()}, ratio_to_rbf=ratios(ms)))
