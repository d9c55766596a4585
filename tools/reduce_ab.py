#!/usr/bin/env python
"""Outputs of every entry point whose kernels sum in one of reduce.hpp's fixed orders, from fixed seeds, as .npy files:

    CIMRGP_LIB_PATH=<library A> python tools/reduce_ab.py dump out_a
    CIMRGP_LIB_PATH=<library B> python tools/reduce_ab.py dump out_b
    python tools/reduce_ab.py compare out_a out_b        (host only)

`compare` views every pair of arrays as integers: two builds of the library that keep the summation orders give the
same bits in every file.  The shapes sit on the boundaries of the row walk (64-column lane stride, 4 rows per workgroup),
of the 1024-thread sums, and of the tiles and slices of the gradient kernels.  Seconds in total.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DTS = ("f64", "f32")


def dump(out_dir):
    import torch

    import cimrgp_amd
    dev = cimrgp_amd.device
    dev.require_gpu()
    os.makedirs(out_dir, exist_ok=True)
    tdt = {"f64": torch.float64, "f32": torch.float32}
    count = [0]

    def save(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            np.save(os.path.join(out_dir, "%s.%d.npy" % (name, i)), t.detach().cpu().numpy())
            count[0] += 1

    def rng(*key):
        return np.random.default_rng([int(k) for k in key])

    def vec(a, dt):
        return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", tdt[dt]).contiguous()

    def padded(a, dt):
        buf = dev.alloc_matrix(a.shape[0], a.shape[1], tdt[dt], "cuda")
        buf.zero_()
        buf[:a.shape[0], :a.shape[1]] = vec(a, dt)
        return buf

    def slabs(a, dt):
        buf = torch.zeros((a.shape[0], a.shape[1], dev.padded_ld(a.shape[2])), dtype=tdt[dt], device="cuda")
        buf[:, :, :a.shape[2]] = vec(a, dt)
        return buf

    rows_n, cols_m, outs_q = (1, 4, 5, 333), (1, 63, 64, 65, 257), (1, 3, 8)
    sums_n = (1, 1023, 1024, 1025, 5000)

    # ---- the sparse row kernels
    for dt, n, m in itertools.product(DTS, rows_n, cols_m):
        g = rng(1, n, m)
        a = g.normal(size=(n, m)) * 0.5 / np.sqrt(m)
        v = g.normal(size=(n, m)) * 0.05 / np.sqrt(m)
        ab, vb = padded(a, dt), padded(v, dt)
        for mode in (0, 1):
            save("lambda_%s_%d_%d_%d" % (dt, n, m, mode), *dev.sparse_lambda(ab, n, m, 1.3, 0.02, mode))
        d = 2
        sa, sw = slabs(g.normal(size=(d + 1, n, m)), dt), slabs(g.normal(size=(d + 1, n, m)), dt)
        for q in outs_q:
            gamma, r = vec(g.normal(size=(m, q)), dt), vec(g.normal(size=(n, q)), dt)
            w = vec(1.0 / (0.02 + g.uniform(0, 1.3, size=n)), dt)
            for acc in (0, 1):
                mean, var = vec(g.normal(size=(n, q)), dt), vec(g.normal(size=n), dt)
                dev.sparse_tail(ab, vb, n, m, gamma, 1.3, 0.25, mean, var, accumulate=bool(acc))
                mg, vg = vec(g.normal(size=(n, d, q)), dt), vec(g.normal(size=(n, d)), dt)
                dev.sparse_tail_grad(sa, sw, n, m, gamma, mg, vg, accumulate=bool(acc))
                save("tail_%s_%d_%d_%d_%d" % (dt, n, m, q, acc), mean, var, mg, vg)
            for mode in (0, 1):
                bad = torch.zeros(1, dtype=torch.int32, device="cuda")
                lm = torch.empty((n, q), dtype=tdt[dt], device="cuda")
                lv = torch.empty(n, dtype=tdt[dt], device="cuda")
                dev.sparse_loo(ab, vb, n, m, gamma, r, 1.3, 0.02, mode, bad, lm, lv)
                save("loo_%s_%d_%d_%d_%d" % (dt, n, m, q, mode), lm, lv, bad,
                     *dev.sparse_grad_rows(vb, n, m, gamma, r, w, mode, 0.02))

    # ---- the 1024-thread sums behind sparse_lambda and sparse_grad_rows
    for dt, n in itertools.product(DTS, sums_n):
        g = rng(2, n)
        m, q = 16, 2
        ab = padded(g.normal(size=(n, m)) * 0.5 / np.sqrt(m), dt)
        gamma, r = vec(g.normal(size=(m, q)), dt), vec(g.normal(size=(n, q)), dt)
        w = vec(1.0 / (0.02 + g.uniform(0, 1.3, size=n)), dt)
        for mode in (0, 1):
            save("sums_%s_%d_%d" % (dt, n, mode), *(dev.sparse_lambda(ab, n, m, 1.3, 0.02, mode)
                                                     + dev.sparse_grad_rows(ab, n, m, gamma, r, w, mode, 0.02)))

    # ---- the pair gradient: one tile, and several tiles and slices
    for dt, (na, nb, d), cov in itertools.product(DTS, ((50, 100, 2), (3001, 257, 3), (4097, 130, 8)), (0, 1, 2, 3)):
        g = rng(3, na, nb)
        xa, xb = vec(g.uniform(-2, 2, size=(na, d)) / np.sqrt(d), dt), vec(g.uniform(-2, 2, size=(nb, d)) / np.sqrt(d), dt)
        gb = padded(g.normal(size=(na, nb)), dt)
        save("pair_%s_%d_%d_%d" % (dt, na, nb, cov), *(dev.cov_pair_grad(xa, xb, gb, 0.7, 1.3, cov=cov)
                                                       + dev.cov_pair_grad_ard(xa, xb, gb, 1.0, 1.3, cov=cov)))

    # ---- block statistics and the log-determinant
    for dt, n in itertools.product(DTS, (1, 1023, 1025, 5000)):
        g = rng(4, n)
        y, fbar = vec(g.normal(size=(n, 3)) + 0.5, dt), vec(0.3 * g.normal(size=(n, 3)), dt)
        lb = dev.alloc_matrix(n, n, tdt[dt], "cuda")
        lb.zero_()
        lb[:n, :n].diagonal().copy_(vec(g.uniform(0.5, 2.0, size=n), dt))
        save("stats_%s_%d" % (dt, n), dev.block_stats(y, fbar), dev.block_stats(y, None), dev.logdet_half(lb, n))

    # ---- the gradient of the log marginal likelihood, plain and ARD
    for dt, n, cov in itertools.product(DTS, (64, 130, 700), (0, 1, 2, 3)):
        g = rng(5, n)
        d, q = 3, 2
        x, alpha = vec(g.uniform(-2, 2, size=(n, d)), dt), vec(g.normal(size=(n, q)), dt)
        kinv = padded(g.normal(size=(n, n)), dt)
        save("lmlgrad_%s_%d_%d" % (dt, n, cov), dev.lml_grad(x, kinv, n, alpha, 0.7, 1.3, 0.05, cov=cov),
             dev.lml_grad_ard(x, kinv, n, alpha, 1.3, 0.05, cov=cov))

    # ---- the layer objective, 3 blocks of 320, plain and ARD
    for dt in DTS:
        g = rng(6)
        batch, n, d, q = 3, 320, 2, 2
        rows = 5 + batch * (n + 3)
        xn = g.uniform(-2, 2, size=(rows, d))
        yn = np.stack([np.sin(2 * xn[:, 0] + c) + 0.3 * xn[:, -1] for c in range(q)], axis=1) + 0.1 * g.normal(size=(rows, q)) + 0.5
        x, y, fbar = vec(xn, dt), vec(yn, dt), vec(0.3 * g.normal(size=(rows, q)), dt)
        starts = torch.tensor([5 + b * (n + 3) for b in range(batch)], dtype=torch.int64, device="cuda")
        ws_bytes = max((dev.potrf_workspace_bytes(n, tdt[dt]) + 15) // 16 * 16, 16)
        for ard in (False, True):
            karena = torch.zeros((batch, n, dev.padded_ld(n)), dtype=tdt[dt], device="cuda")
            kinv = torch.zeros_like(karena)
            ws = torch.zeros((batch, ws_bytes), dtype=torch.uint8, device="cuda")
            info = torch.zeros(batch, dtype=torch.int32, device="cuda")
            out = torch.zeros((batch, d + 3 if ard else 4), dtype=torch.float64, device="cuda")
            if ard:
                dev.layer_lml_grad_ard(x, y, fbar, starts, n, 1.3, 0.05, None, karena, kinv, ws, info, out)
            else:
                dev.layer_lml_grad(x, y, fbar, starts, n, 0.7, 1.3, 0.05, None, karena, kinv, ws, info, out)
            save("layerlml_%s_%d" % (dt, ard), out, info)

    # ---- diag(K^-1), the solves and the thin update (potrs), from a factored Gram matrix
    for dt, n in itertools.product(DTS, (300, 700)):
        g = rng(7, n)
        x = vec(g.uniform(-2, 2, size=(n, 2)), dt)
        lb = dev.rbf_gram(x, 0.7, 1.3, 0.05, lower_only=True)
        ws, info = dev.potrf(lb, n)
        rhs = vec(g.normal(size=(n, 3)), dt)
        z = dev.potrs(lb, n, ws, rhs, want_z=True)
        save("solve_%s_%d" % (dt, n), dev.kinv_diag(lb, n, ws, 1 << 22), rhs, z, info)

    # ---- the reduced-rank moments: several workgroups
    for dt, m in itertools.product(DTS, (3, 20)):
        g = rng(8, m)
        n, q = 20000, 2
        x = vec(g.uniform(-1, 1, size=(n, 1)), dt)
        y, fbar, fvar = vec(g.normal(size=(n, q)), dt), vec(0.3 * g.normal(size=(n, q)), dt), vec(g.uniform(0, 1, size=n), dt)
        bm = dev.basis_moments(x, [1.5], m, y, fbar, fvar, 0.1 * g.normal(size=(q, m)))
        for i, a in enumerate((bm.proj, bm.colsum, bm.colsum2, bm.resid_sum, np.array([bm.resid_sq, bm.fvar_sum]))):
            np.save(os.path.join(out_dir, "moments_%s_%d.%d.npy" % (dt, m, i)), np.asarray(a))
            count[0] += 1

    # ---- the predictive gradient's contraction and the prediction tail
    for dt, d in itertools.product(DTS, (1, 3)):
        g = rng(9, d)
        ns, n, q = 9, 70, 2
        x, xs = vec(g.uniform(-2, 2, size=(n, d)), dt), vec(g.uniform(-2, 2, size=(ns, d)), dt)
        alpha, beta = vec(g.normal(size=(n, q)), dt), padded(g.normal(size=(ns, n)), dt)
        mg = torch.empty((ns, d, q), dtype=tdt[dt], device="cuda")
        vg = torch.empty((ns, d), dtype=tdt[dt], device="cuda")
        dev.cov_predict_grad(x, alpha, xs, 0.7, 1.3, beta, mg, vg, cov=2)
        save("predgrad_%s_%d" % (dt, d), mg, vg)
    for dt, n in itertools.product(DTS, (1, 2, 511, 513)):
        g = rng(10, n)
        ns, q = 7, 3
        wb, z = padded(g.normal(size=(ns, n)), dt), vec(g.normal(size=(n, q)), dt)
        mean = torch.empty((ns, q), dtype=tdt[dt], device="cuda")
        var = torch.empty(ns, dtype=tdt[dt], device="cuda")
        dev.predict_from_w(wb, ns, n, z, 1.3, 0.02, vec(g.normal(size=q), dt), mean, var)
        save("fromw_%s_%d" % (dt, n), mean, var)
    print("reduce_ab: %d arrays written to %s" % (count[0], out_dir))


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if names_a != names_b or not names_a:
        print("reduce_ab: the two directories do not hold the same files")
        return 1
    differing = []
    for name in names_a:
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        bits = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
        same = a.dtype == b.dtype and a.shape == b.shape
        if not (same and np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))):
            differing.append(name)
    print("reduce_ab: %d arrays compared, %d differ%s"
          % (len(names_a), len(differing), (": " + ", ".join(differing[:20])) if differing else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
