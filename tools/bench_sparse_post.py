"""Timing of the sparse GP's posterior queries (include/cimrgp_sparse_post.h) on one GPU: FP64, device events after warm-up,
median of --reps, the routes alternating in one process, at n = 65 536, m = 1000, d = 2, q = 1, N* = 100 000, RBF, FITC:
  * SparseBlock.predict_grad against SparseBlock.predict (mean and variance) at the same test points: by flop count d + 1
    predictions; central differences would cost 2 d + 1;
  * SparseBlock.loo against predict at the training inputs: about one prediction;
  * the adding SYRK of cimrgp_sparse_joint_cov against cimrgp_syrk_lower at ns = 4096, K = 1000: the joint call (Gram,
    subtraction, addition) against cimrgp_cov_gram + cimrgp_syrk_lower (Gram, subtraction); the difference is the addition;
  * SparseBlock.joint with 8 and 256 sample columns at N* = 4096 (covariance, factorisation, normals, product).
Nothing is judged.  One JSON line on stdout, appended to the file named by the first argument if given."""
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
tdt = torch.float64


def timed(fns, reps, warmup=2):
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


n, m, d, q, ns = 65536, 1000, 2, 1, 100000
rng = np.random.default_rng(n + d)
xh = rng.uniform(-2, 2, size=(n, d))
yh = (np.sin(2 * xh).sum(axis=1) + 0.1 * rng.normal(size=n))[:, None]
x, y = dev.to_device(xh, tdt, "cuda"), dev.to_device(yh, tdt, "cuda")
z = x[torch.as_tensor(np.random.RandomState(0).permutation(n)[:m]).to("cuda")].contiguous()
xs = dev.to_device(rng.uniform(-2.2, 2.2, size=(ns, d)), tdt, "cuda")
ell, sf, noise = 0.4 * np.sqrt(d), 1.0, 0.01
blk = SparseBlock(x, z, RBFKernel(l=ell, sf=sf, noise=noise), 'fitc', 1e-6).fit(y)

mean, var = torch.empty((ns, q), dtype=tdt, device="cuda"), torch.empty(ns, dtype=tdt, device="cuda")
mg, vg = torch.empty((ns, d, q), dtype=tdt, device="cuda"), torch.empty((ns, d), dtype=tdt, device="cuda")
tmean, tvar = torch.empty((n, q), dtype=tdt, device="cuda"), torch.empty(n, dtype=tdt, device="cuda")
t_pred, t_grad, t_pred_train, t_loo = timed((lambda: blk.predict(xs, mean, var), lambda: blk.predict_grad(xs, mg, vg),
                                             lambda: blk.predict(x, tmean, tvar), lambda: blk.loo(y, tmean, tvar)), args.reps)

# the adding SYRK beside the subtracting one: the same operands, C of the joint call's pitch
nj = 4096
xj = xs[:nj].contiguous()
ld = dev.joint_ld(m, tdt)
astar = torch.empty((nj, ld), dtype=tdt, device="cuda")
astar.normal_()
astar.mul_(0.01)
wstar = astar.clone()
cbuf = torch.empty((nj, dev.joint_ld(nj, tdt)), dtype=tdt, device="cuda")


def gram_and_sub():
    dev.rbf_gram(xj, ell, sf, 0.0, lower_only=True, out=cbuf)
    dev.syrk_lower(cbuf, astar, nj, m)


t_joint, t_gram_sub, t_gram, t_sub = timed((lambda: dev.sparse_joint_cov(xj, ell, sf, 0.0, astar, wstar, m, cbuf), gram_and_sub,
                                            lambda: dev.rbf_gram(xj, ell, sf, 0.0, lower_only=True, out=cbuf),
                                            lambda: dev.syrk_lower(cbuf, astar, nj, m)), args.reps)
s8, s256 = torch.zeros((8, nj), dtype=tdt, device="cuda"), torch.zeros((256, nj), dtype=tdt, device="cuda")
cov_out = torch.zeros((nj, nj), dtype=tdt, device="cuda")
t_s8, t_s256, t_cov = timed((lambda: blk.joint(xj, samples=s8), lambda: blk.joint(xj, samples=s256),
                             lambda: blk.joint(xj, cov_out=cov_out)), args.reps)

line = json.dumps({"case": "sparse_post", "device": torch.cuda.get_device_name(0), "dtype": "f64", "approximation": "fitc", "cov": "rbf",
                   "n": n, "m": m, "d": d, "q": q, "ns": ns, "predict_ms": t_pred, "predict_grad_ms": t_grad,
                   "predict_grad_over_predict": t_grad / t_pred, "predict_at_training_inputs_ms": t_pred_train, "loo_ms": t_loo,
                   "loo_over_predict": t_loo / t_pred_train, "joint_ns": nj, "joint_cov_call_ms": t_joint,
                   "gram_plus_syrk_lower_ms": t_gram_sub, "gram_ms": t_gram, "syrk_lower_ms": t_sub,
                   "add_syrk_ms": t_joint - t_gram_sub, "add_syrk_over_syrk_lower": (t_joint - t_gram_sub) / t_sub,
                   "samples_8_ms": t_s8, "samples_256_ms": t_s256, "joint_covariance_ms": t_cov})
print(line, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
