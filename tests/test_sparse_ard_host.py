"""CPU tests of the ARD length-scales of the sparse GP (include/cimrgp_sparse_ard.h): the header's symbols, every refusal of
cimrgp_cov_pair_grad_ard that precedes a HIP call, its scratch formula, the refusals of SparseBlock(lengthscales=) and of the
plugins' ARD keyword, and the two oracle forms of tests/sparse_ard_numpy.py against each other, against central differences
and, at equal length-scales, against the isotropic oracle of tests/sparse_grad_numpy.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import sparse_ard_numpy as sa
import sparse_grad_numpy as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, M, Q = 300, 40, 2
ELLS = (0.7, 1.3, 2.1)
SF, NOISE, EPS = 1.3, 0.02, 1e-6
#: the agreement DESIGN.md records for the isotropic pair of oracle forms and for central differences, asserted at 10 x
THETA_LEVEL, Z_LEVEL, CENTRAL_LEVEL = 1.6e-13, 8.2e-12, 3.7e-9
MARGIN = 10.0


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_sparse_ard_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse_ard.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_cov_pair_grad_ard", "cimrgp_cov_pair_grad_ard_scratch_bytes"]
    assert sorted(_lib.SPARSE_ARD_SIGNATURES) == names
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SPARSE_ARD_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.SPARSE_ARD_SIGNATURES[name][0], name
    # the twin's arguments, one for one
    assert _lib.SPARSE_ARD_SIGNATURES["cimrgp_cov_pair_grad_ard"] == _lib.SPARSE_GRAD_SIGNATURES["cimrgp_cov_pair_grad"]
    assert '#include "cimrgp_sparse_ard.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    # every header beside cimrgp.h is a dependency of every object: the build script takes them by pattern
    build = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    assert "for h in *.hpp ../../include/*.h" in build and '"$h" -nt "$f.o"' in build


def test_pair_grad_ard_scratch_bytes_by_formula():
    lib = _lib.load()
    assert sa.pair_scratch_bytes(65536, 1024, 2) == 8 * 128 * 8 * (128 * 2 + 3)
    for na, nb, d in ((65536, 1024, 2), (4097, 130, 3), (1, 1, 1), (255, 100, 2), (3001, 257, 8), (1 << 24, 1 << 20, 8)):
        assert int(lib.cimrgp_cov_pair_grad_ard_scratch_bytes(na, nb, d)) == sa.pair_scratch_bytes(na, nb, d), (na, nb, d)
        # d - 1 more doubles per workgroup than the twin
        assert (sa.pair_scratch_bytes(na, nb, d) - sg.pair_scratch_bytes(na, nb, d)
                == 8 * sg.pair_slices(na, nb)[0] * ((nb + 127) // 128) * (d - 1))
    for bad in ((0, 16, 1), (16, 0, 1), ((1 << 24) + 1, 16, 1), (16, (1 << 20) + 1, 1), (16, 16, 0), (16, 16, 9)):
        assert int(lib.cimrgp_cov_pair_grad_ard_scratch_bytes(*bad)) == 0, bad


# ---- refusals --------------------------------------------------------------------------------------------------------
NAME = 'cimrgp_cov_pair_grad_ard'
BASE = [('dtype', 1), ('cov', 0), ('xa', 'P'), ('na', 600), ('xb', 'P'), ('nb', 100), ('d', 2), ('g', 'P'), ('ldg', 112), ('ell', 0.7),
        ('sf2', 1.3), ('scale', 1.0), ('accumulate', 0), ('sums', 'P'), ('db', 'P'), ('scratch', 'P'), ('scratch_bytes', 1 << 20),
        ('stream', None)]

ROWS = [
    ({'dtype': 7}, -1, 'cimrgp_cov_pair_grad_ard: unknown dtype'),
    ({'cov': 4}, -1, 'cimrgp_cov_pair_grad_ard: unknown covariance'),
    ({'cov': -1}, -1, 'cimrgp_cov_pair_grad_ard: unknown covariance'),
    ({'xa': None}, -1, 'cimrgp_cov_pair_grad_ard: null pointer'),
    ({'xb': None}, -1, 'cimrgp_cov_pair_grad_ard: null pointer'),
    ({'g': None}, -1, 'cimrgp_cov_pair_grad_ard: null pointer'),
    ({'scratch': None}, -1, 'cimrgp_cov_pair_grad_ard: null pointer'),
    ({'na': 0}, -1, 'cimrgp_cov_pair_grad_ard: na must be in [1, 16777216]'),
    ({'na': (1 << 24) + 1}, -1, 'cimrgp_cov_pair_grad_ard: na must be in [1, 16777216]'),
    ({'nb': 0}, -1, 'cimrgp_cov_pair_grad_ard: nb must be in [1, 1048576]'),
    ({'nb': (1 << 20) + 1, 'ldg': 1 << 21}, -1, 'cimrgp_cov_pair_grad_ard: nb must be in [1, 1048576]'),
    ({'d': 0}, -1, 'cimrgp_cov_pair_grad_ard: input dimension must be in [1, 8]'),
    ({'d': 9}, -1, 'cimrgp_cov_pair_grad_ard: input dimension must be in [1, 8]'),
    ({'ldg': 99}, -1, 'cimrgp_cov_pair_grad_ard: leading dimension too small'),
    ({'ell': 0.0}, -1, 'cimrgp_cov_pair_grad_ard: kernel parameters must be positive'),
    ({'sf2': -1.0}, -1, 'cimrgp_cov_pair_grad_ard: kernel parameters must be positive'),
    ({'scratch': 'P+4'}, -1, 'cimrgp_cov_pair_grad_ard: scratch must be 8-byte aligned'),
    ({'scratch_bytes': 6215}, -1, 'cimrgp_cov_pair_grad_ard: scratch too small'),
    # what is enough for the twin (6192 bytes) is not enough here
    ({'scratch_bytes': 6192}, -1, 'cimrgp_cov_pair_grad_ard: scratch too small'),
    ({'dtype': 7, 'cov': 9, 'xa': None, 'na': 0, 'd': 0}, -1, 'cimrgp_cov_pair_grad_ard: unknown dtype'),
    ({'sums': None, 'db': None, 'scratch_bytes': 0}, -1, 'cimrgp_cov_pair_grad_ard: scratch too small'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [{'sums': None, 'db': None}, {'sums': None, 'db': None, 'scratch_bytes': 6216}]


def _args(broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+4": p + 4}


def test_pair_grad_ard_refusals_status_and_text():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE]
    assert len(BASE) == len(_lib.SPARSE_ARD_SIGNATURES[NAME][1])
    assert sa.pair_scratch_bytes(600, 100, 2) == 6216 and sg.pair_scratch_bytes(600, 100, 2) == 6192
    for broken, status, text in ROWS:
        assert broken and set(broken) <= set(keys), broken
        rc = getattr(lib, NAME)(*_args(broken, stand_in))
        print(broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), broken


def test_the_refusal_rows_are_the_twins_under_the_new_name():
    import test_sparse_grad_host as twin
    mine = {(tuple(sorted(b.items())), st, tx) for b, st, tx in ROWS}
    for name, broken, status, text in twin.ROWS:
        if name != 'cimrgp_cov_pair_grad':
            continue
        if broken == {'scratch_bytes': 6191}:
            broken = {'scratch_bytes': 6215}
        assert (tuple(sorted(broken.items())), status, text.replace('cimrgp_cov_pair_grad', NAME)) in mine, broken
    assert BASE == twin.BASE['cimrgp_cov_pair_grad']


def test_pair_grad_ard_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for broken in NO_WORK:
        assert getattr(lib, NAME)(*_args(broken, stand_in)) == 0, broken


# ---- SparseBlock(lengthscales=) and the plugins' ARD= -----------------------------------------------------------------
def test_block_constructor_refusals():
    torch = pytest.importorskip("torch")
    from cimrgp_amd.KernelClass import DenseMaternKernel, RBFKernel
    from cimrgp_amd.Sparse import SparseBlock
    x, z = torch.zeros((10, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64)
    unit = RBFKernel(l=1.0, sf=1.3, noise=0.02)
    blk = SparseBlock(x, z, unit, 'fitc', 1e-6, False, (0.5, 1.0, 2.0))              # the new argument is the last
    assert np.array_equal(blk.lengthscales, [0.5, 1.0, 2.0]) and blk.x is x
    assert torch.equal(blk.cov.scale, torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64))
    assert torch.equal(blk.cov.inputs(x + 1.0), torch.tensor([[2.0, 1.0, 0.5]] * 10, dtype=torch.float64))
    plain = SparseBlock(x, z, unit)
    assert plain.lengthscales is None and plain.cov.scale is None
    assert plain.cov.inputs(plain.x) is plain.x and plain.cov.inputs(plain.z) is plain.z      # the caller's tensors, no copies
    assert plain._xs is plain.x and plain._zs is plain.z
    for bad in ((0.5, 1.0), (0.5, 1.0, 2.0, 3.0), 0.5, [[0.5, 1.0, 2.0]], (0.5, 0.0, 2.0), (0.5, -1.0, 2.0), (0.5, np.nan, 2.0),
                (0.5, np.inf, 2.0)):
        with pytest.raises(ValueError, match="lengthscales"):
            SparseBlock(x, z, unit, lengthscales=bad)
    for kernel in (RBFKernel(l=0.5, sf=1.3, noise=0.02), DenseMaternKernel(nu=1.5, l=2.0, sf=1.3, noise=0.02)):
        with pytest.raises(ValueError, match="l = 1.0"):
            SparseBlock(x, z, kernel, lengthscales=(0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match="device_noise"):
        SparseBlock(x, z, unit, device_noise=True, lengthscales=(0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match="device_noise"):
        SparseBlock(x, z, RBFKernel(l=1.0, sf=1.3), device_noise=True, lengthscales=(0.5, 1.0, 2.0))


def test_plugin_keyword_validation():
    from cimrgp_amd import SGP_FITC, SparseGP, SparseGP_RBF
    for cls in (SparseGP, SGP_FITC, SparseGP_RBF):
        g = cls()
        assert g.ARD is False and g.lengthscales is None and g.kernel.l == 1.0
        assert cls(lengthscale=0.5).kernel.l == 0.5
        with pytest.raises(ValueError, match="ARD=True"):
            cls(lengthscale=(0.7, 1.3))
        with pytest.raises(ValueError, match="ARD=True"):
            cls(lengthscale=[0.7], ARD=False)
        with pytest.raises(ValueError, match="lengthscale"):
            cls(lengthscale=[[0.7, 1.3]], ARD=True)
        # with ARD=True the kernel is built at l = 1, so the constructor checks the user's values itself
        for bad in (0.0, -1.0, np.nan, np.inf, (0.7, 0.0), (0.7, -1.3), (np.nan, 1.3), (0.7, np.inf), ()):
            with pytest.raises(ValueError, match="lengthscale must be"):
                cls(lengthscale=bad, ARD=True)
        for ls in (0.5, (0.7, 1.3)):
            g = cls(lengthscale=ls, ARD=True, optimize=True, jac='analytic', optimize_inducing=True)
            assert g.ARD is True and g.kernel.l == 1.0 and g.lengthscales is None
        # a wrong length is refused by fit, before anything else
        g = cls(lengthscale=(0.7, 1.3), ARD=True)
        with pytest.raises(ValueError, match="2 entries.*3 dimensions"):
            g.fit([np.random.default_rng(0).normal(size=(20, 3)), np.random.default_rng(1).normal(size=(20, 1))])
    # ARD is the last keyword of all three; positional callers are unaffected
    import inspect
    for cls in (SparseGP, SGP_FITC, SparseGP_RBF):
        assert list(inspect.signature(cls.__init__).parameters)[-1] == 'ARD'
    assert SGP_FITC(10, 0.5, 2.0).kernel.l == 0.5 and SparseGP(10, 'vfe', 0.5).approximation == 'vfe'


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
def test_pair_reference_is_the_projects_formulae_in_either_precision(cov):
    """sparse_ard_numpy.k_and_g restates grad_numpy.kcov / g_of so that numpy.longdouble can evaluate them: in FP64 it
    agrees with them to a few roundings, in extended precision with its own FP64 form; summed over e the per-dimension
    sums are sparse_grad_numpy.pair_grad's sum of G dk/dlog l, and sum k and db are its."""
    from grad_numpy import g_of, kcov
    rng = np.random.default_rng(cov)
    xa, xb, g = rng.uniform(-2, 2, size=(50, 3)), rng.uniform(-2, 2, size=(20, 3)), rng.normal(size=(50, 20))
    xa[:20] = xb                                        # r = 0 pairs
    k, gr, _ = sa.k_and_g(xa, xb, cov, 0.7, 1.3)
    assert _rel(k, kcov(xa, xb, cov, 0.7, 1.3)) <= 1e-14 and _rel(gr, g_of(xa, xb, cov, 0.7, 1.3)) <= 1e-14
    kl, gl, _ = sa.k_and_g(xa, xb, cov, 0.7, 1.3, np.longdouble)
    assert _rel(np.asarray(kl, dtype=np.float64), k) <= 1e-14 and _rel(np.asarray(gl, dtype=np.float64), gr) <= 1e-14
    for ft in (np.float64, np.longdouble):
        (s, db), (smag, mag) = sa.pair_grad_ard(xa, xb, g, cov, 0.7, 1.3, scale=-2.0, ft=ft)
        (s2, db2), (smag2, mag2) = sg.pair_grad(xa, xb, g, cov, 0.7, 1.3, scale=-2.0)
        assert abs(s[0] - s2[0]) <= 1e-13 * smag2[0] and abs(s[1:].sum() - s2[1]) <= 1e-13 * smag2[1]
        assert abs(smag[1:].sum() - smag2[1]) <= 1e-13 * smag2[1] and (np.abs(db - db2) <= 1e-13 * mag2).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [2, 3])
def test_the_two_ard_oracle_forms_agree_and_match_central_differences(d, cov, mode):
    """The NumPy chain on pre-scaled inputs, torch FP64 CPU autograd with a length-scale vector and central differences
    (step 1e-5) of sparse_numpy.woodbury, at 10 x the levels DESIGN.md records for the isotropic pair of forms."""
    ells = np.array(ELLS[:d])
    x, z, r = sg.problem(N, M, d, seed=N + M + d + cov, q=Q)
    lml, dtheta, dz = sa.chain(x, z, r, cov, ells, SF, NOISE, EPS, mode)
    la, ta, za = sa.autograd(x, z, r, cov, ells, SF, NOISE, EPS, mode)
    central = sa.central_theta(x, z, r, cov, ells, SF, NOISE, EPS, mode)
    print("d %d cov %d mode %d: value %.1e  theta %.1e  Z %.1e  central %.1e"
          % (d, cov, mode, abs(la - lml) / abs(lml), _rel(dtheta, ta), _rel(dz, za), _rel(central, ta)))
    assert dtheta.shape == ta.shape == central.shape == (d + 2,) and dz.shape == za.shape == (M, d)
    assert abs(la - lml) <= 1e-12 * abs(lml)
    assert _rel(dtheta, ta) <= MARGIN * THETA_LEVEL
    assert _rel(dz, za) <= MARGIN * Z_LEVEL
    assert _rel(central, ta) <= MARGIN * CENTRAL_LEVEL


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
def test_equal_lengthscales_sum_to_the_isotropic_derivative(cov, mode):
    """With l_e = l for all e the derivatives w.r.t. log l_e add up to the isotropic d F / d log l, and everything else is
    the isotropic oracle's.  The two are autograd of the same chain up to where the division by l happens: all held to
    1e-12 (DESIGN.md records 7e-16 for theta, 3.3e-14 for Z and 1.9e-15 for the value)."""
    d, ell = 3, 0.7
    x, z, r = sg.problem(N, M, d, seed=N + M + d + cov, q=Q)
    l_iso, t_iso, z_iso = sg.autograd(x, z, r, cov, ell, SF, NOISE, EPS, mode)
    l_ard, t_ard, z_ard = sa.autograd(x, z, r, cov, np.full(d, ell), SF, NOISE, EPS, mode)
    folded = np.array([t_ard[0], t_ard[1:1 + d].sum(), t_ard[-1]])
    print("cov %d mode %d: value %.1e theta %.1e Z %.1e" % (cov, mode, abs(l_ard - l_iso) / abs(l_iso), _rel(folded, t_iso),
                                                           _rel(z_ard, z_iso)))
    assert abs(l_ard - l_iso) <= 1e-12 * abs(l_iso)
    assert _rel(folded, t_iso) <= 1e-12
    assert _rel(z_ard, z_iso) <= 1e-12
