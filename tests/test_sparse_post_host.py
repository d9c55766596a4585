"""CPU tests of the sparse GP's posterior queries (include/cimrgp_sparse_post.h; DESIGN.md, "Posterior queries of the sparse
GP"): the header's symbols, every refusal of the four entry points that precedes a HIP call, the refusals of the new
SparseBlock and plugin methods, and the oracle of tests/sparse_post_numpy.py: its Woodbury forms against the dense n x n
definition, and its gradients against central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import sparse_post_numpy as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, M, Q = 300, 40, 2
ELL, SF, NOISE, EPS = 0.7, 1.3, 0.02, 1e-6
#: the agreement of the oracle's gradients with central differences (h = 1e-5) measured in NumPy over the 16 cases below
#: (DESIGN.md records them), asserted at 10 x.  The figure is Matern 1/2's at d = 2 (the third derivatives of |x - z| grow
#: like 1 / r^2 towards an inducing input, so a fixed step is worth fewer digits there); the other three covariances
#: measure 1.3e-9.
CENTRAL_LEVEL = 3.9e-7
MARGIN = 10.0


def test_sparse_post_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse_post.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_cov_cross_grad", "cimrgp_sparse_joint_cov", "cimrgp_sparse_loo", "cimrgp_sparse_tail_grad"]
    assert sorted(_lib.SPARSE_POST_SIGNATURES) == names
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SPARSE_POST_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.SPARSE_POST_SIGNATURES[name][0], name
        # one ctypes entry per argument of the declaration
        decl = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, text).group(1)
        assert len(decl.split(",")) == len(_lib.SPARSE_POST_SIGNATURES[name][1]), name
    # the leading arguments of the cross-covariance call are cimrgp_cov_cross's, one for one
    assert _lib.SPARSE_POST_SIGNATURES["cimrgp_cov_cross_grad"][1][:11] == _lib.SIGNATURES["cimrgp_cov_cross"][1][:11]
    assert '#include "cimrgp_sparse_post.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    build = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    # every header beside cimrgp.h is a dependency of every object: the build script takes them by pattern
    assert " sparse_post " in build and "for h in *.hpp ../../include/*.h" in build and '"$h" -nt "$f.o"' in build


# ---- refusals --------------------------------------------------------------------------------------------------------
BASE = {
    'cimrgp_cov_cross_grad': [('dtype', 1), ('cov', 0), ('xa', 'P'), ('na', 600), ('xb', 'P'), ('nb', 100), ('d', 2), ('ell', 0.7),
                              ('sf2', 1.3), ('out', 'P'), ('ldo', 112), ('slab_stride', 600 * 112), ('stream', None)],
    'cimrgp_sparse_tail_grad': [('dtype', 1), ('a', 'P'), ('w', 'P'), ('ns', 600), ('m', 100), ('d', 2), ('ld', 112),
                                ('slab_stride', 600 * 112), ('gamma', 'P'), ('q', 2), ('mean_grad', 'P'), ('var_grad', 'P'),
                                ('accumulate', 0), ('stream', None)],
    'cimrgp_sparse_loo': [('dtype', 1), ('a', 'P'), ('v', 'P'), ('n', 600), ('m', 100), ('ld', 112), ('gamma', 'P'), ('r', 'P'),
                          ('q', 2), ('sf2', 1.3), ('noise', 0.02), ('mode', 0), ('loo_mean', 'P'), ('loo_var', 'P'), ('bad', 'P'),
                          ('stream', None)],
    'cimrgp_sparse_joint_cov': [('dtype', 1), ('cov', 0), ('xs', 'P'), ('ns', 600), ('d', 2), ('ell', 0.7), ('sf2', 1.3),
                                ('diag', 0.0), ('astar', 'P'), ('wstar', 'P'), ('m', 100), ('ld', 112), ('c', 'P'), ('ldc', 608),
                                ('cws', 'P'), ('cws_bytes', 1 << 30), ('info', 'P'), ('stream', None)],
}

CG, TG, LO, JC = 'cimrgp_cov_cross_grad', 'cimrgp_sparse_tail_grad', 'cimrgp_sparse_loo', 'cimrgp_sparse_joint_cov'
ROWS = [
    (CG, {'dtype': 7}, -1, 'cimrgp_cov_cross_grad: unknown dtype'),
    (CG, {'cov': 4}, -1, 'cimrgp_cov_cross_grad: unknown covariance'),
    (CG, {'cov': -1}, -1, 'cimrgp_cov_cross_grad: unknown covariance'),
    (CG, {'xa': None}, -1, 'cimrgp_cov_cross_grad: null pointer'),
    (CG, {'xb': None}, -1, 'cimrgp_cov_cross_grad: null pointer'),
    (CG, {'out': None}, -1, 'cimrgp_cov_cross_grad: null pointer'),
    (CG, {'na': -1}, -1, 'cimrgp_cov_cross_grad: na and nb must be in [0, 2^30)'),
    (CG, {'na': 1 << 30, 'slab_stride': 1 << 40}, -1, 'cimrgp_cov_cross_grad: na and nb must be in [0, 2^30)'),
    (CG, {'nb': -1}, -1, 'cimrgp_cov_cross_grad: na and nb must be in [0, 2^30)'),
    (CG, {'nb': 1 << 30, 'ldo': 1 << 30, 'slab_stride': 1 << 50}, -1, 'cimrgp_cov_cross_grad: na and nb must be in [0, 2^30)'),
    (CG, {'d': 0}, -1, 'cimrgp_cov_cross_grad: input dimension must be in [1, 8]'),
    (CG, {'d': 9}, -1, 'cimrgp_cov_cross_grad: input dimension must be in [1, 8]'),
    (CG, {'ell': 0.0}, -1, 'cimrgp_cov_cross_grad: kernel parameters must be positive'),
    (CG, {'sf2': -1.0}, -1, 'cimrgp_cov_cross_grad: kernel parameters must be positive'),
    (CG, {'ldo': 99}, -1, 'cimrgp_cov_cross_grad: leading dimension too small'),
    (CG, {'slab_stride': 599 * 112 + 99}, -1, 'cimrgp_cov_cross_grad: slab stride too small'),
    (CG, {'na': 1 << 26, 'nb': 1 << 26, 'ldo': 1 << 26, 'slab_stride': 1 << 60}, -1, 'cimrgp_cov_cross_grad: grid too large'),
    (CG, {'dtype': 7, 'cov': 9, 'xa': None, 'na': -1, 'd': 0}, -1, 'cimrgp_cov_cross_grad: unknown dtype'),
    (TG, {'dtype': 7}, -1, 'cimrgp_sparse_tail_grad: unknown dtype'),
    (TG, {'w': None}, -1, 'cimrgp_sparse_tail_grad: null pointer'),
    (TG, {'a': None}, -1, 'cimrgp_sparse_tail_grad: null pointer (a)'),
    (TG, {'gamma': None}, -1, 'cimrgp_sparse_tail_grad: null pointer (gamma)'),
    (TG, {'ns': -1}, -1, 'cimrgp_sparse_tail_grad: bad dimensions'),
    (TG, {'ns': 1 << 30, 'slab_stride': 1 << 40}, -1, 'cimrgp_sparse_tail_grad: bad dimensions'),
    (TG, {'m': 0}, -1, 'cimrgp_sparse_tail_grad: bad dimensions'),
    (TG, {'ld': 99}, -1, 'cimrgp_sparse_tail_grad: bad dimensions'),
    (TG, {'d': 0}, -1, 'cimrgp_sparse_tail_grad: input dimension must be in [1, 8]'),
    (TG, {'d': 9}, -1, 'cimrgp_sparse_tail_grad: input dimension must be in [1, 8]'),
    (TG, {'q': 0}, -1, 'cimrgp_sparse_tail_grad: number of outputs must be in [1, 8]'),
    (TG, {'q': 9}, -1, 'cimrgp_sparse_tail_grad: number of outputs must be in [1, 8]'),
    (TG, {'slab_stride': 599 * 112 + 99}, -1, 'cimrgp_sparse_tail_grad: slab stride too small'),
    (LO, {'dtype': 7}, -1, 'cimrgp_sparse_loo: unknown dtype'),
    (LO, {'a': None}, -1, 'cimrgp_sparse_loo: null pointer'),
    (LO, {'v': None}, -1, 'cimrgp_sparse_loo: null pointer'),
    (LO, {'gamma': None}, -1, 'cimrgp_sparse_loo: null pointer'),
    (LO, {'r': None}, -1, 'cimrgp_sparse_loo: null pointer'),
    (LO, {'bad': None}, -1, 'cimrgp_sparse_loo: null pointer'),
    (LO, {'n': -1}, -1, 'cimrgp_sparse_loo: bad dimensions'),
    (LO, {'n': 1 << 31}, -1, 'cimrgp_sparse_loo: bad dimensions'),
    (LO, {'m': 0}, -1, 'cimrgp_sparse_loo: bad dimensions'),
    (LO, {'ld': 99}, -1, 'cimrgp_sparse_loo: bad dimensions'),
    (LO, {'q': 0}, -1, 'cimrgp_sparse_loo: number of outputs must be in [1, 8]'),
    (LO, {'q': 9}, -1, 'cimrgp_sparse_loo: number of outputs must be in [1, 8]'),
    (LO, {'mode': 2}, -1, 'cimrgp_sparse_loo: mode must be 0 (FITC) or 1 (VFE)'),
    (LO, {'sf2': 0.0}, -1, 'cimrgp_sparse_loo: sf2 and noise must be positive'),
    (LO, {'noise': 0.0}, -1, 'cimrgp_sparse_loo: sf2 and noise must be positive'),
    (JC, {'dtype': 7}, -1, 'cimrgp_sparse_joint_cov: unknown dtype'),
    (JC, {'cov': 4}, -1, 'cimrgp_sparse_joint_cov: unknown covariance'),
    (JC, {'xs': None}, -1, 'cimrgp_sparse_joint_cov: null pointer'),
    (JC, {'astar': None}, -1, 'cimrgp_sparse_joint_cov: null pointer'),
    (JC, {'wstar': None}, -1, 'cimrgp_sparse_joint_cov: null pointer'),
    (JC, {'c': None}, -1, 'cimrgp_sparse_joint_cov: null pointer'),
    (JC, {'info': None}, -1, 'cimrgp_sparse_joint_cov: null pointer (info)'),
    (JC, {'ns': -1}, -1, 'cimrgp_sparse_joint_cov: bad dimensions'),
    (JC, {'ns': 1 << 30, 'ldc': 1 << 30}, -1, 'cimrgp_sparse_joint_cov: bad dimensions'),
    (JC, {'m': 0}, -1, 'cimrgp_sparse_joint_cov: bad dimensions'),
    (JC, {'d': 0}, -1, 'cimrgp_sparse_joint_cov: input dimension must be in [1, 8]'),
    (JC, {'d': 9}, -1, 'cimrgp_sparse_joint_cov: input dimension must be in [1, 8]'),
    (JC, {'ell': 0.0}, -1, 'cimrgp_sparse_joint_cov: kernel parameters must be positive'),
    (JC, {'sf2': 0.0}, -1, 'cimrgp_sparse_joint_cov: kernel parameters must be positive'),
    (JC, {'ld': 98}, -1, 'cimrgp_sparse_joint_cov: leading dimension too small'),
    (JC, {'ldc': 598}, -1, 'cimrgp_sparse_joint_cov: leading dimension too small'),
    (JC, {'ld': 111}, -1, 'cimrgp_sparse_joint_cov: leading dimensions must be multiples of 16 bytes'),
    (JC, {'ldc': 601}, -1, 'cimrgp_sparse_joint_cov: leading dimensions must be multiples of 16 bytes'),
    (JC, {'m': 4, 'ld': 8}, -1, 'cimrgp_sparse_joint_cov: leading dimension of A* and W* must span at least 128 bytes'),
    (JC, {'dtype': 0, 'm': 4, 'ld': 28}, -1, 'cimrgp_sparse_joint_cov: leading dimension of A* and W* must span at least 128 bytes'),
    (JC, {'astar': 'P+8'}, -1, 'cimrgp_sparse_joint_cov: pointers must be 16-byte aligned'),
    (JC, {'wstar': 'P+8'}, -1, 'cimrgp_sparse_joint_cov: pointers must be 16-byte aligned'),
    (JC, {'c': 'P+8'}, -1, 'cimrgp_sparse_joint_cov: pointers must be 16-byte aligned'),
    (JC, {'cws': 'P+8'}, -1, 'cimrgp_sparse_joint_cov: pointers must be 16-byte aligned'),
    (JC, {'cws_bytes': 1000}, -1, 'cimrgp_sparse_joint_cov: factor workspace too small'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [
    (CG, {'na': 0, 'slab_stride': 0}), (CG, {'nb': 0}),
    (TG, {'ns': 0, 'slab_stride': 0}), (TG, {'mean_grad': None, 'var_grad': None}),
    (TG, {'mean_grad': None, 'var_grad': None, 'a': None, 'gamma': None, 'q': 0}),
    (LO, {'n': 0}),
    (JC, {'ns': 0}), (JC, {'ns': 0, 'cws': None, 'info': None, 'cws_bytes': 0}),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+8": p + 8}


def test_sparse_post_refusals_status_and_text():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name in BASE:
        assert len(BASE[name]) == len(_lib.SPARSE_POST_SIGNATURES[name][1]), name
    for name, broken, status, text in ROWS:
        assert broken and set(broken) <= {k for k, _ in BASE[name]}, broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_every_check_of_the_four_entry_points_has_a_row():
    """Each CIMRGP_REQUIRE text of sparse_post.hip's entry points occurs in the table under its function's name."""
    src = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "sparse_post.hip")).read()
    ext = src[src.index('extern "C" {'):]
    seen = {(name, text.split(': ', 1)[1]) for name, _, _, text in ROWS}
    for name in BASE:
        body = ext[ext.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        for what in re.findall(r'CIMRGP_REQUIRE\(.*?, fn,\s*"([^"]+)"\);', body, re.S):
            assert (name, what) in seen, (name, what)


def test_sparse_post_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name, broken in NO_WORK:
        assert getattr(lib, name)(*_args(name, broken, stand_in)) == 0, (name, broken, _lib.last_error())


# ---- SparseBlock and the plugins ---------------------------------------------------------------------------------------
def test_block_methods_refuse_before_fit_and_for_a_layers_block():
    torch = pytest.importorskip("torch")
    from cimrgp_amd.KernelClass import RBFKernel
    from cimrgp_amd.Sparse import SparseBlock
    x, z = torch.zeros((10, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64)
    xs, r = torch.zeros((5, 3), dtype=torch.float64), torch.zeros((10, 2), dtype=torch.float64)
    blk = SparseBlock(x, z, RBFKernel(l=0.7, sf=1.3, noise=0.02))
    for call in (lambda b: b.predict_grad(xs, None, None), lambda b: b.loo(r, None, None), lambda b: b.joint(xs)):
        with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
            call(blk)
    for kernel in (RBFKernel(l=0.7, sf=1.3, noise=0.02), RBFKernel(l=0.7, sf=1.3)):
        layer = SparseBlock(x, z, kernel, device_noise=True)
        for call in (lambda b: b.predict_grad(xs, None, None), lambda b: b.loo(r, None, None), lambda b: b.joint(xs)):
            with pytest.raises(TypeError, match="not yet supported"):
                call(layer)
    # chunk rows of the gradient count 2 (d + 1) slabs, the prediction's count 2
    assert blk.chunk_rows(1 << 20) == max(256, (1 << 20) // (2 * 16 * 8) // 256 * 256)
    assert blk.grad_chunk_rows(1 << 20) == max(256, (1 << 20) // (2 * 4 * 16 * 8) // 256 * 256)
    assert blk.grad_chunk_rows(1) == 256


def test_plugin_methods_refuse_before_fit_and_keep_every_signature():
    import inspect
    from cimrgp_amd import GP_RBF, SGP_FITC, SparseGP, SparseGP_RBF
    xs = np.zeros((3, 2))
    for cls in (SparseGP, SGP_FITC, SparseGP_RBF):
        g = cls()
        for name, args in (("predictive_gradients", (xs,)), ("leave_one_out", ()), ("loo_log_predictive_density", ()),
                           ("predict_with_covariance", (xs,)), ("posterior_samples_f", (xs,))):
            with pytest.raises(RuntimeError, match=r"call fit\(\) before"):
                getattr(g, name)(*args)
            # the exact plugin's parameters, in its order, lead the sparse method's
            exact = list(inspect.signature(getattr(GP_RBF, name)).parameters)
            assert list(inspect.signature(getattr(cls, name)).parameters)[:len(exact)] == exact, name
        assert inspect.signature(cls.posterior_samples_f).parameters['size'].default == 1
        assert inspect.signature(cls.posterior_samples_f).parameters['seed'].default == 0
        assert list(inspect.signature(cls.predict_with_variance).parameters) == ['self', 'test_data', 'include_noise', 'budget_bytes']


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _fit(d, cov, mode, n=N, m=M):
    x, z, r, xs = sp.problem(n, m, d, seed=n + m + d + cov, q=Q)
    return sp.Fit(x, z, r, cov, ELL, SF, NOISE, EPS, mode), xs


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [2, 3])
def test_woodbury_forms_equal_the_dense_definition(d, cov, mode):
    """LOO through the leverage against K~^-1, the joint covariance against Q** - Q*f K~^-1 Qf* + (K** - Q**), the
    gradients against those of Q*f K~^-1 r and sf - Q*f K~^-1 Qf*: 1e-10."""
    fit, xs = _fit(d, cov, mode)
    lm, lv, h = sp.loo(fit)
    dm, dv = sp.loo_dense(fit)
    c, _, _ = sp.joint_cov(fit, xs)
    cd = sp.joint_cov_dense(fit, xs)
    print("d %d cov %d mode %d: loo mean %.1e var %.1e  cov %.1e  max h %.3f"
          % (d, cov, mode, sp.rel(lm, dm), sp.rel(lv, dv), sp.rel(c, cd), h.max()))
    assert h.max() < 0.99
    assert sp.rel(lm, dm) <= 1e-10 and sp.rel(lv, dv) <= 1e-10
    assert sp.rel(c, cd) <= 1e-10
    (mg, vg), (dg, dv) = sp.predict_grad(fit, xs), sp.predict_grad_dense(fit, xs)
    print("    gradients: mean %.1e var %.1e" % (sp.rel(mg, dg), sp.rel(vg, dv)))
    assert sp.rel(mg, dg) <= 1e-10 and sp.rel(vg, dv) <= 1e-10
    # the diagonal is the predictive variance of sparse_numpy.woodbury, the mean W* gamma its mean
    _, mean, var = sp.woodbury(fit.x, fit.z, fit.r, cov, ELL, SF, NOISE, EPS, mode, xs)
    assert sp.rel(np.diag(c), var) <= 1e-12
    assert sp.rel(fit.star(xs)[1] @ fit.gamma, mean) <= 1e-12


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [2, 3])
def test_oracle_gradients_match_central_differences(d, cov, mode):
    fit, xs = _fit(d, cov, mode)
    mg, vg = sp.predict_grad(fit, xs)
    cm, cv = sp.central(fit, xs, 1e-5)
    print("d %d cov %d mode %d: mean %.1e var %.1e" % (d, cov, mode, sp.rel(cm, mg), sp.rel(cv, vg)))
    assert mg.shape == (xs.shape[0], d, Q) and vg.shape == (xs.shape[0], d)
    assert sp.rel(cm, mg) <= MARGIN * CENTRAL_LEVEL
    assert sp.rel(cv, vg) <= MARGIN * CENTRAL_LEVEL


def test_cross_grad_slabs_are_the_projects_k_and_g_and_vanish_at_r_zero_for_matern12():
    rng = np.random.default_rng(0)
    xb = rng.uniform(-2, 2, size=(20, 3))
    xa = np.concatenate([xb[:7], rng.uniform(-2, 2, size=(30, 3))])
    for cov in range(4):
        s = sp.cross_grad(xa, xb, cov, ELL, SF)
        assert s.shape == (4, 37, 20) and np.array_equal(s[0], sp.kcov(xa, xb, cov, ELL, SF))
        for i in range(7):
            assert (s[1:, i, i] == 0).all()             # df = 0; Matern 1/2: g = 0 too
        h = 1e-6
        for e in range(3):
            xp, xm = xa.copy(), xa.copy()
            xp[:, e] += h
            xm[:, e] -= h
            fd = (sp.kcov(xp, xb, cov, ELL, SF) - sp.kcov(xm, xb, cov, ELL, SF)) / (2 * h)
            mask = np.ones_like(fd, dtype=bool)
            mask[np.arange(7), np.arange(7)] = False     # the kink of Matern 1/2
            assert np.abs(fd - s[1 + e])[mask].max() <= 1e-6 * np.abs(s[1 + e]).max()
