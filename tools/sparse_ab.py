#!/usr/bin/env python
"""Results of the sparse GP from fixed seeds, as .npy files, for comparing two commits of the PYTHON layer bit for bit:

    CIMRGP_LIB_PATH=<one libcimrgp.so> python <checkout A>/tools/sparse_ab.py dump out_a
    CIMRGP_LIB_PATH=<the same library> python <checkout B>/tools/sparse_ab.py dump out_b
    python tools/sparse_ab.py compare out_a out_b        (host only)

`dump` imports the package that lies beside the copy of this script that is run, so the same script copied into two
checkouts dumps each one's Sparse.py / KernelClass.py against one library.  `compare` views every pair of arrays as
integers and requires equality: a rewrite of the host side that keeps every device call and every torch operation gives
the same bits in every file.

Block level, per arm (plain, ARD, linear, ARD + linear), FITC and VFE, f64 and f32, RBF and Matern 3/2: the LML, predict
(with and without the noise, in two chunks), lml_grad's (lml, dtheta, dZ) and grad_check and, for the arms without a
linear term, predict_grad, loo, and joint's covariance and samples.  Plugin level: SparseGP(ARD) and SparseGP_RBFLinear
learning their hyper-parameters and Z for 3 iterations; the seven queries of SGP_FITC(ARD); SVIGP_RBF at fixed
hyper-parameters and after 3 iterations (params, elbo_grad, predict, predict_with_variance); BGPLVM on the shared-variance
and the per-row route and after 3 iterations (elbo, kl_divergence, predict with and without test_var,
predict_with_variance); GP_RBF(ARD)'s joint covariance and samples.  Model level: two layers, the second sparse over an ARD base.
K() of both kernel classes, isotropic and ARD.  n = 300, m = 70, d = 3, q = 2, ns = 300: across the 64-column lane
stride, the 256-row slice and chunk boundaries and one 128-column tile of the pair contraction.  Seconds in total.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N, M, D, Q, NS = 300, 70, 3, 2, 300
ELLS, LINEAR = np.array([0.7, 1.3, 2.1]), np.array([0.5, 0.2, 0.1])
SF, NOISE = 1.3, 0.02
JITTER = {"f64": 1e-6, "f32": 1e-4}
ARMS = ("plain", "ard", "linear", "ard_linear")


def _data(n=N, ns=NS, d=D, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d))
    y = np.stack([np.sin(2 * x[:, 0] + c) + 0.4 * x[:, -1] for c in range(Q)], axis=1) + 0.1 * rng.normal(size=(n, Q))
    return x, y, rng.uniform(-2.2, 2.2, size=(ns, d))


def dump(out_dir):
    import torch

    import cimrgp_amd as ca
    from cimrgp_amd.Sparse import SparseBlock
    dev = ca.device
    dev.require_gpu()
    os.makedirs(out_dir, exist_ok=True)
    count = [0]

    def save(name, *arrays):
        torch.cuda.synchronize()
        for i, a in enumerate(arrays):
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.atleast_1d(np.asarray(a, dtype=np.float64))
            np.save(os.path.join(out_dir, "%s.%d.npy" % (name, i)), a)
            count[0] += 1

    # ---- block level
    xh, yh, xsh = _data()
    for arm, mode, dt, matern in itertools.product(ARMS, ("fitc", "vfe"), ("f64", "f32"), (False, True)):
        tdt = dev.as_torch_dtype(dt)
        x, r, xs = (dev.to_device(a, tdt, "cuda") for a in (xh, yh - yh.mean(axis=0), xsh))
        z = x[torch.as_tensor(np.random.RandomState(1).permutation(N)[:M]).to("cuda")].contiguous()
        ell = 1.0 if "ard" in arm else 0.9
        kernel = ca.DenseMaternKernel(nu=1.5, l=ell, sf=SF, noise=NOISE) if matern else ca.RBFKernel(l=ell, sf=SF, noise=NOISE)
        kw = dict(lengthscales=ELLS) if "ard" in arm else {}
        if "linear" in arm:
            kw["linear"] = LINEAR
        tag = "block_%s_%s_%s_%s" % (arm, mode, dt, "m32" if matern else "rbf")

        def block():
            return SparseBlock(x, z, kernel, mode, JITTER[dt], **kw)

        def out(*shape):
            return torch.full(shape, 7.0, dtype=tdt, device="cuda")

        blk = block().fit(r)
        save(tag + "_lml", blk.log_marginal_likelihood())
        budget = 2 * dev.padded_ld(M) * x.element_size() * 256         # chunks of 256 rows: two for ns = 300
        for noise in (False, True):
            save(tag + "_predict%d" % noise, *blk.predict(xs, out(NS, Q), out(NS), include_noise=noise, budget_bytes=budget))
        save(tag + "_predict_mean_only", blk.predict(xs, out(NS, Q), None, budget_bytes=budget)[0])
        for want_z in (True, False):
            g = block()
            lml, dtheta, dz = g.lml_grad(r, want_z=want_z)
            save(tag + "_grad%d" % want_z, lml, dtheta, g.grad_check["closed"], g.grad_check["pairwise"], *([dz] if want_z else []))
        if "linear" in arm:
            continue
        save(tag + "_predict_grad", *blk.predict_grad(xs, out(NS, D, Q), out(NS, D), budget_bytes=1))
        save(tag + "_loo", *blk.loo(r, out(N, Q), out(N), budget_bytes=budget))
        cov = torch.zeros((NS, NS), dtype=tdt, device="cuda")
        samples = torch.zeros((3, NS), dtype=tdt, device="cuda")
        save(tag + "_joint", blk.joint(xs, cov_out=cov, include_noise=True), cov, blk.joint(xs, samples=samples, seed=5), samples)

    # ---- plugin level: hyper-parameters and Z learned for 3 iterations
    xp, yp, xsp = _data(seed=1)
    for name, gp in (("sparsegp_ard", ca.SparseGP(num_inducing=M, ARD=True, optimize=True, jac="analytic", optimize_inducing=True,
                                                  max_iters=3)),
                     ("rbflinear", ca.SparseGP_RBFLinear(num_inducing=M, optimize=True, jac="analytic", max_iters=3))):
        gp.fit([xp, yp])
        save("plugin_" + name, gp.optimizer_result.x, *gp.predict_with_variance(xsp), gp.inducing_inputs)

    # ---- plugin level: every query of a sparse plugin, the variational and the uncertain-input plugins, the exact plugin's joint
    budget = 2 * dev.padded_ld(M) * 8 * 256                              # float64 chunks of 256 rows: two for ns = 300
    gp = ca.SGP_FITC(num_inducing=M, ARD=True, lengthscale=ELLS)
    gp.fit([xp, yp])
    save("plugin_fitc_predict", gp.predict(xsp), *gp.predict_with_variance(xsp, include_noise=True, budget_bytes=budget))
    save("plugin_fitc_gradients", *gp.predictive_gradients(xsp, budget_bytes=budget))
    save("plugin_fitc_loo", *gp.leave_one_out(budget_bytes=budget), gp.loo_log_predictive_density(budget_bytes=budget))
    save("plugin_fitc_joint", *gp.predict_with_covariance(xsp), gp.posterior_samples_f(xsp, size=2, seed=5), gp.inducing_inputs)
    for optimize in (False, True):
        gp = ca.SVIGP_RBF(num_inducing=M, optimize=optimize, max_iters=3)
        gp.fit([xp, yp])
        save("plugin_svigp_optimize%d" % optimize, gp.params, *gp.elbo_grad(), gp.predict(xsp),
             *gp.predict_with_variance(xsp, budget_bytes=budget), gp.inducing_inputs)
    x_var_rows = np.random.default_rng(3).uniform(0.0, 0.05, size=xp.shape)
    for name, kw in (("shared", dict(X_var=0.02)), ("rows", dict(X_var=x_var_rows)), ("optimized", dict(optimize=True, max_iters=3))):
        gp = ca.BGPLVM(num_inducing=M, **kw)
        gp.fit([xp, yp])
        save("plugin_bgplvm_" + name, gp.elbo(), gp.kl_divergence(), gp.predict(xsp),
             *gp.predict_with_variance(xsp, include_noise=True, budget_bytes=budget), gp.predict(xsp, test_var=0.03, budget_bytes=budget),
             gp.predict(xsp, test_var=np.full(xsp.shape, 0.03), budget_bytes=budget), gp.lengthscales, gp.inducing_inputs)
    gp = ca.GP_RBF(lengthscale=0.9, ARD=True, optimize=False)
    gp.fit([xp, yp])
    save("plugin_gp_rbf_ard", *gp.predict_with_covariance(xsp), gp.posterior_samples_f(xsp, size=2, seed=5))

    # ---- model level: two layers, the second sparse over an ARD base
    from cimrgp_amd.Inputs import space_filling_order
    xm, ym, xsm = _data(n=600, d=2, seed=2)
    order = space_filling_order(xm)
    xm, ym, xsm = xm[order], ym[order], xsm[space_filling_order(xsm)]
    kernels = [ca.RBFKernel(l=1.0, sf=1.0, noise=0.05),
               ca.SparseKernel(ca.RBFKernel(l=[0.4, 0.9], sf=0.5, noise=0.05), num_inducing=M, approximation="vfe")]
    model = ca.MultiResolutionGaussianProcess([xm, ym], index_set_obj=ca.IndexSetUniform(600, 1, 2), spectral_density_obj=kernels)
    model.fit()
    save("model", *model.get_predicted_mean_and_var(xsm, ca.IndexSetUniform(NS, 1, 2)))

    # ---- K() of both kernel classes
    for name, k in (("rbf", ca.RBFKernel(l=0.9, sf=SF)), ("rbf_ard", ca.RBFKernel(l=ELLS, sf=SF)),
                    ("m32", ca.DenseMaternKernel(nu=1.5, l=0.9, sf=SF)), ("m32_ard", ca.DenseMaternKernel(nu=1.5, l=ELLS, sf=SF))):
        save("K_" + name, k.K(xh), k.K(xsh[:50], xh))
    print("sparse_ab: %d arrays written to %s" % (count[0], out_dir))


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if names_a != names_b or not names_a:
        print("sparse_ab: the two directories do not hold the same files")
        return 1
    differing = []
    for name in names_a:
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        bits = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
        same = a.dtype == b.dtype and a.shape == b.shape
        if not (same and np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))):
            differing.append(name)
    print("sparse_ab: %d arrays compared, %d differ%s"
          % (len(names_a), len(differing), (": " + ", ".join(differing[:20])) if differing else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
