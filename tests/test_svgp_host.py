"""Host tests (no GPU) of the variational sparse GP (include/cimrgp_svgp.h, cimrgp_amd/SVGP.py, the SVIGP_RBF plugin; DESIGN.md,
"Variational sparse GP with a Student-t likelihood"): the oracle of tests/svgp_numpy.py against itself, against central
differences and against the VFE bound of tests/sparse_linear_numpy.py; the device's chain rule replayed on the CPU
(tests/svgp_mirror.py, through SVGP's own m x m algebra) against autograd; the parameter vector of Hyper; and the header,
the table, the library's symbols, the refusals of the entry points and the plugin's constructor rules."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import sparse_linear_numpy as sl
import svgp_mirror as sm
import svgp_numpy as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 300, 40
SF, S2, NU, WHITE, EPS = 1.3, 0.05, 3.0, 0.01, 1e-6
ELLS, LINS = np.array([0.7, 1.3, 0.9]), np.array([0.5, 0.2, 0.35])


def _gap(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _case(d, q, linear=True, seed=0):
    x, z, y = so.problem(N, M, d, q, 10 * d + q + seed)
    theta = so.theta_of(ELLS[:d], SF, S2, LINS[:d] if linear else None)
    mu, p = so.perturbed_posterior(M, q, 3)
    return x, z, y, theta, mu, p, dict(white=WHITE, eps=EPS, linear=linear)


@pytest.mark.parametrize("lik", ["gaussian", "student_t"])
@pytest.mark.parametrize("d,q", [(1, 1), (2, 2), (3, 1)])
def test_the_oracles_two_forms_agree(lik, d, q):
    """The dense form (n x n, q(u) unwhitened) and the whitened chain: the gap is the oracle's own error, what the GPU tests
    multiply by 100.  Recorded at n = 300, m = 40, ARD + linear + white: F 1.2e-15, gradients at most 2.3e-14, prediction 8.7e-15."""
    x, z, y, theta, mu, p, kw = _case(d, q)
    dense = so.elbo("dense", x, z, y, 0, theta, mu, p, lik, nu=NU, **kw)
    chain = so.elbo("chain", x, z, y, 0, theta, mu, p, lik, nu=NU, **kw)
    xs = np.random.default_rng(1).uniform(-1.1, 1.1, size=(50, d))
    pd, pc = so.predict("dense", x, z, xs, 0, theta, mu, p, **kw), so.predict("chain", x, z, xs, 0, theta, mu, p, **kw)
    gaps = [abs(dense[0] - chain[0]) / abs(dense[0])] + [_gap(chain[i], dense[i]) for i in (1, 2, 3)] + [_gap(pc[0], pd[0]), _gap(pc[1], pd[1])]
    print("oracle %s d %d q %d: dense vs chain F %.1e theta %.1e mu %.1e P %.1e mean %.1e var %.1e; min v %.4f"
          % ((lik, d, q) + tuple(gaps) + (so.min_variance(x, z, 0, theta, mu, p, **kw),)))
    assert max(gaps) <= 1e-11
    assert so.min_variance(x, z, 0, theta, mu, p, **kw) > 0


@pytest.mark.parametrize("lik", ["gaussian", "student_t"])
def test_autograd_agrees_with_central_differences(lik):
    """Step 1e-5 over every hyper-parameter and a spread of the entries of mu and of P's lower triangle.  Central differences
    of a sum of this size are good to ~1e-9 of the largest gradient entry; 1e-6 is asked."""
    x, z, y, theta, mu, p, kw = _case(2, 2)
    _, dth, dmu, dp = so.elbo("chain", x, z, y, 0, theta, mu, p, lik, nu=NU, **kw)
    nt, tri = theta.size, M * (M + 1) // 2
    idx = np.unique(np.concatenate([np.arange(nt), nt + np.arange(0, 2 * M, 9), nt + 2 * M + np.arange(0, 2 * tri, 97)]))
    cd, pack = so.central(x, z, y, 0, theta, mu, p, lik, step=1e-5, indices=idx, nu=NU, **kw)
    grad = pack(dth, dmu, dp)
    gap = float(np.abs(cd - grad[idx]).max() / np.abs(grad).max())
    print("central differences %s: %.2e of the largest entry %.1f over %d entries" % (lik, gap, np.abs(grad).max(), idx.size))
    assert gap <= 1e-6


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_at_the_gaussian_optimum_the_bound_is_the_vfe_bound_and_the_posteriors_gradient_vanishes(d, q):
    """P = L_B, mu = L_B^-T gamma of the VFE fit with noise s2.  With white = 0 the ELBO is the VFE bound of
    tests/sparse_linear_numpy.py as it stands; with white > 0 that bound is taken at the jitter eps + white / sf and loses the
    white variance's share of the trace term, n q white / (2 s2)."""
    x, z, y, theta, _, _, kw = _case(d, q)
    for white in (0.0, WHITE):
        kw["white"] = white
        mu, p = so.gaussian_optimum(x, z, y, 0, theta, **kw)
        f, _, dmu, dp = so.elbo("chain", x, z, y, 0, theta, mu, p, "gaussian", **kw)
        vfe = sl.woodbury(x, z, y, 0, ELLS[:d], SF, S2, EPS + white / SF, 1, LINS[:d])[0] - 0.5 * N * q * white / S2
        scale = np.abs(so.elbo("chain", x, z, y, 0, theta, *so.perturbed_posterior(M, q, 3), "gaussian", **kw)[2]).max()
        print("gaussian optimum d %d q %d white %.2f: F - VFE %.2e, |dmu| %.2e |dP| %.2e of %.1f"
              % (d, q, white, abs(f - vfe) / abs(vfe), np.abs(dmu).max() / scale, np.abs(dp).max() / scale, scale))
        assert abs(f - vfe) <= 1e-11 * abs(vfe)
        assert np.abs(dmu).max() <= 1e-10 * scale and np.abs(dp).max() <= 1e-10 * scale


def test_twenty_nodes_against_forty_for_the_student_t():
    """Reported: the gap gives the floor of any comparison across node counts (none is made elsewhere: the device and the
    oracle both use H = 20).  Measured at these shapes: F 1.7e-4 relative, the gradients up to 7.6e-3 of their largest entry --
    the Student-t's log density is not a polynomial, and sqrt(2 v) is several noise scales wide at this perturbed posterior."""
    for d, q in ((1, 1), (2, 2), (3, 2)):
        x, z, y, theta, mu, p, kw = _case(d, q)
        f20 = so.elbo("chain", x, z, y, 0, theta, mu, p, "student_t", nu=NU, nodes=20, **kw)
        f40 = so.elbo("chain", x, z, y, 0, theta, mu, p, "student_t", nu=NU, nodes=40, **kw)
        gaps = [abs(f20[0] - f40[0]) / abs(f40[0])] + [_gap(f20[i], f40[i]) for i in (1, 2, 3)]
        print("H = 20 vs 40, d %d q %d: F %.2e theta %.2e mu %.2e P %.2e" % ((d, q) + tuple(gaps)))
        assert np.isfinite(gaps).all() and gaps[0] < 0.05
        g20 = so.elbo("chain", x, z, y, 0, theta, mu, p, "gaussian", nodes=20, **kw)[0]
        g40 = so.elbo("chain", x, z, y, 0, theta, mu, p, "gaussian", nodes=40, **kw)[0]
        assert abs(g20 - g40) <= 1e-12 * abs(g40)           # a quadratic: exact at any H >= 2


@pytest.mark.parametrize("lik", ["gaussian", "student_t"])
@pytest.mark.parametrize("d,q,linear", [(1, 2, False), (2, 1, True), (3, 2, True)])
def test_the_devices_chain_rule_on_the_cpu_against_autograd(lik, d, q, linear):
    """tests/svgp_mirror.py: g1, g2 by their closed forms, SVGP.column_terms and SVGP.kuu_weight for the m x m algebra, the pair
    contractions with the weights G_fu, G_uu, t held fixed -- against autograd of the dense definition."""
    x, z, y, theta, mu, p, kw = _case(d, q, linear)
    dense = so.elbo("dense", x, z, y, 2, theta, mu, p, lik, nu=NU, **kw)
    mirror = sm.elbo_grad(x, z, y, 2, theta, mu, p, lik, nu=NU, **kw)
    gaps = [abs(mirror[0] - dense[0]) / abs(dense[0])] + [_gap(mirror[i], dense[i]) for i in (1, 2, 3)]
    print("mirror %s d %d q %d linear %d: F %.1e theta %.1e mu %.1e P %.1e" % ((lik, d, q, linear) + tuple(gaps)))
    assert max(gaps) <= 1e-11


def test_the_parameter_vector_round_trips_and_its_gradient_is_the_chain_rule():
    from cimrgp_amd import Hyper
    mu, p = so.perturbed_posterior(5, 2, 1)
    vec = Hyper.pack_posterior(mu, p)
    assert vec.shape == (2 * 5 + 2 * 15,)
    mu2, p2 = Hyper.unpack_posterior(vec, 2, 5)
    assert np.array_equal(mu2, mu) and np.allclose(p2, p, rtol=1e-15, atol=0) and (np.triu(p2, 1) == 0).all()
    assert np.array_equal(vec[10:15][[0, 2]], np.log([p[0, 0, 0], p[0, 1, 1]])) and vec[11] == p[0, 1, 0]
    rng = np.random.default_rng(0)
    dmu, dp = rng.normal(size=mu.shape), np.tril(rng.normal(size=p.shape))
    g = Hyper.posterior_gradient(dmu, dp, p)
    f = lambda v: (Hyper.unpack_posterior(v, 2, 5)[0] * dmu).sum() + (Hyper.unpack_posterior(v, 2, 5)[1] * dp).sum()
    for k in range(vec.size):
        hi, lo = vec.copy(), vec.copy()
        hi[k] += 1e-6
        lo[k] -= 1e-6
        assert abs((f(hi) - f(lo)) / 2e-6 - g[k]) <= 1e-8 * max(1.0, abs(g[k]))
    # the driver climbs a concave quadratic in all three parts
    target = np.array([0.3, -0.2])

    def bowl(theta, m_, p_):
        return (-((theta - target) ** 2).sum() - ((m_ - mu) ** 2).sum() - ((p_ - p) ** 2).sum(),
                -2 * (theta - target), -2 * (m_ - mu), -2 * np.tril(p_ - p))

    res, theta, mu3, p3 = Hyper.maximize_elbo(bowl, np.zeros(2), np.zeros_like(mu), np.stack([np.eye(5)] * 2), 200)
    assert np.allclose(theta, target, atol=1e-5) and np.allclose(mu3, mu, atol=1e-5) and np.allclose(p3, p, atol=1e-5)


# ---- the header, the table and the library ---------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    from cimrgp_amd import _lib
    from test_abi_signatures_host import prototypes
    assert _lib.HEADERS["cimrgp_svgp.h"] is _lib.SVGP_SIGNATURES and list(_lib.HEADERS)[-1] == "cimrgp_svgp.h"
    names = [name for name, _, _ in prototypes("cimrgp_svgp.h")]
    assert sorted(names) == sorted(_lib.SVGP_SIGNATURES) == ["cimrgp_svgp_moments", "cimrgp_svgp_moments_scratch_bytes", "cimrgp_svgp_rows"]
    text = open(os.path.join(ROOT, "include", "cimrgp_svgp.h")).read()
    assert "#define CIMRGP_LIK_GAUSSIAN %d" % _lib.LIK_GAUSSIAN in text and "#define CIMRGP_LIK_STUDENT_T %d" % _lib.LIK_STUDENT_T in text
    assert "#define CIMRGP_SVGP_SUM_CHUNK %d" % _lib.SVGP_SUM_CHUNK in text
    assert '#include "cimrgp_svgp.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SVGP_SIGNATURES[name][1]
    symbols = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert " T %s\n" % name in symbols, name
    assert lib.cimrgp_svgp_moments_scratch_bytes(_lib.F64, 5000, 130, 2) == lib.cimrgp_wsyrk_tn_scratch_bytes(_lib.F64, 5000, 130, 2) > 0
    assert lib.cimrgp_svgp_moments_scratch_bytes(_lib.F64, 0, 130, 2) == 0


def test_refusals_name_the_call():
    """Every argument is checked before any device work: host addresses stand in for the buffers."""
    from cimrgp_amd import _lib as L
    lib = L.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    base = dict(dtype=L.F64, a=p, w=p, n=2, m=4, ld=4, gamma=p, kdiag=p, y=p, ys=1, nodes=p, h=4, lik=0, s2=0.1, nu=3.0)
    rows = [(dict(dtype=7), "unknown dtype"), (dict(a=None), "null pointer"), (dict(nodes=None), "null pointer"),
            (dict(n=0), "bad dimensions"), (dict(n=1 << 31), "bad dimensions"), (dict(ld=3), "bad dimensions"),
            (dict(ys=0), "y_stride must be positive"),
            (dict(h=0), "number of nodes must be in [1, 64]"), (dict(h=65), "number of nodes must be in [1, 64]"),
            (dict(lik=2), "unknown likelihood"), (dict(s2=0.0), "the likelihood's scale must be positive"),
            (dict(lik=1, nu=0.0), "the degrees of freedom must be positive")]
    for broken, text in rows:
        k = dict(base, **broken)
        rc = lib.cimrgp_svgp_rows(k["dtype"], k["a"], k["w"], k["n"], k["m"], k["ld"], k["gamma"], k["kdiag"], k["y"], k["ys"], k["nodes"],
                                  k["h"], k["lik"], k["s2"], k["nu"], p, p, p, p, None, None, None)
        assert rc < 0 and L.last_error() == "cimrgp_svgp_rows: " + text, broken
    rc = lib.cimrgp_svgp_rows(L.F64, p, p, 2, 4, 4, p, p, p, 1, p, 4, 0, 0.1, 3.0, p, p, p, p, p, None, None)
    assert rc < 0 and L.last_error() == "cimrgp_svgp_rows: null pointer (scratch)"
    for broken, text in [(dict(q=9), "number of outputs must be in [1, 8]"), (dict(nbytes=8), "scratch too small"),
                         (dict(a=None), "null pointer"), (dict(g=None), "null pointer (g)"), (dict(n=0), "n must be in [1, 16777216]"),
                         (dict(lda=3), "leading dimension too small"), (dict(dtype=7), "unknown dtype")]:
        k = dict(dict(dtype=L.F64, a=p, n=2, m=4, lda=4, w=p, r=p, q=1, c=p, ldc=4, g=p, scratch=p, nbytes=1 << 20), **broken)
        rc = lib.cimrgp_svgp_moments(k["dtype"], k["a"], k["n"], k["m"], k["lda"], k["w"], k["r"], k["q"], k["c"], k["ldc"], k["g"],
                                     k["scratch"], k["nbytes"], None)
        assert rc < 0 and L.last_error() == "cimrgp_svgp_moments: " + text, broken
    # the twin keeps its own name
    rc = lib.cimrgp_wsyrk_tn(L.F64, p, 2, 4, 4, p, p, 9, 0.0, p, 4, p, p, 1 << 20, None)
    assert rc < 0 and L.last_error() == "cimrgp_wsyrk_tn: number of outputs must be in [1, 8]"


# ---- the block's and the plugin's rules -------------------------------------------------------------------------------------
def test_block_constructor_rules():
    import torch
    import cimrgp_amd as ca
    x, z = torch.zeros((10, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64)
    k = ca.RBFKernel(l=1.0, sf=1.0)
    sig = inspect.signature(ca.SVGPBlock.__init__)
    assert list(sig.parameters)[1:] == ["x", "z", "kernel", "likelihood", "deg_free", "scale", "white", "jitter", "lengthscales",
                                        "linear", "nodes"]
    assert sig.parameters["likelihood"].default == "student_t" and sig.parameters["deg_free"].default == 3.0
    assert sig.parameters["white"].default == 0.01 and sig.parameters["jitter"].default == 1e-6
    for kw in (dict(likelihood="laplace"), dict(scale=0.0), dict(deg_free=0.0), dict(white=-1.0), dict(jitter=-1.0), dict(nodes=65),
               dict(lengthscales=[1.0]), dict(linear=[1.0, -1.0])):
        with pytest.raises(ValueError):
            ca.SVGPBlock(x, z, k, **kw)
    with pytest.raises(ValueError):
        ca.SVGPBlock(x, z[:, :1], k)
    with pytest.raises(TypeError, match="not yet supported"):
        ca.SVGPBlock(x.float(), z.float(), k)
    blk = ca.SVGPBlock(x, z, k, "gaussian", linear=[0.5, 0.25])
    assert blk.lik == ca._lib.LIK_GAUSSIAN and blk.n == 10 and blk.m == 4 and blk.nodes.shape == (40,)
    with pytest.raises(RuntimeError):
        blk.predict(x)
    with pytest.raises(ValueError):
        blk.elbo_grad(torch.zeros((10, 1), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.float64),
                      torch.zeros((1, 4, 4), dtype=torch.float64))
    xw, ww = np.polynomial.hermite.hermgauss(20)
    from cimrgp_amd.SVGP import hermite_nodes
    assert np.array_equal(hermite_nodes(), np.concatenate([xw, ww]))


def test_plugin_constructor_and_refusals():
    import cimrgp_amd as ca
    assert "SVIGP_RBF" in ca.__all__ and "SVGPBlock" in ca.__all__ and ca.SVIGP_RBF.name == "SVIGP_RBF"
    sig = inspect.signature(ca.SVIGP_RBF.__init__)
    assert list(sig.parameters)[1:] == ["num_inducing", "lengthscale", "variance", "linear_variance", "white_variance", "likelihood",
                                        "deg_free", "nu", "Z", "seed", "jitter", "dtype", "device", "optimize", "max_iters", "ARD", "linear"]
    defaults = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert defaults == dict(num_inducing=100, lengthscale=1., variance=1., linear_variance=1., white_variance=0.01,
                            likelihood="student_t", deg_free=3., nu=None, Z=None, seed=0, jitter=1e-6, dtype="f64", device=None,
                            optimize=True, max_iters=1000, ARD=True, linear=True)
    for kw in (dict(likelihood="laplace"), dict(num_inducing=0), dict(lengthscale=0.0), dict(lengthscale=[1.0, 2.0]), dict(variance=-1.0),
               dict(linear_variance=0.0), dict(deg_free=0.0), dict(white_variance=-0.1), dict(jitter=-1.0), dict(nu=2.0),
               dict(dtype="f16")):
        with pytest.raises(ValueError):
            ca.SVIGP_RBF(**kw)
    with pytest.raises(TypeError, match="not yet supported"):
        ca.SVIGP_RBF(dtype="f32")
    gp = ca.SVIGP_RBF(num_inducing=7, seed=3)
    assert isinstance(gp, ca.RegressionMethod) and gp.block is None and gp.optimizer_result is None
    assert np.array_equal(gp.inducing_draw(20), np.random.RandomState(3).permutation(20)[:7])
    for call in (gp.elbo, gp.elbo_grad, lambda: gp._predict(np.zeros((2, 1)))):
        with pytest.raises(RuntimeError):
            call()
    xs = np.zeros((3, 1))
    for call in (lambda: gp.predictive_gradients(xs), lambda: gp.leave_one_out(), lambda: gp.loo_log_predictive_density(),
                 lambda: gp.predict_with_covariance(xs), lambda: gp.posterior_samples_f(xs)):
        with pytest.raises(TypeError, match="not yet supported"):
            call()
