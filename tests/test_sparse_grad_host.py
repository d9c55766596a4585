"""CPU tests of the gradients of the sparse objective (include/cimrgp_sparse_grad.h): the header's symbols, the scratch
formula, the two oracle forms of tests/sparse_grad_numpy.py against each other and against central differences, the
closed form of d F / d log sf, every refusal that precedes a HIP call, and the plugin's keyword validation."""
import ctypes
import os
import re

import numpy as np
import pytest

from cimrgp_amd import _lib

import sparse_grad_numpy as sg
import sparse_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the check of the issue: n, m, q, the parameters, and the agreement levels it reports (asserted at 10 x)
N, M, Q = 300, 40, 2
ELL, SF, NOISE, EPS = 0.7, 1.3, 0.02, 1e-6
THETA_LEVEL, Z_LEVEL, Z_LEVEL_RBF_1D, CENTRAL_LEVEL, VALUE_LEVEL = 1.7e-13, 2e-11, 2.3e-9, 1.2e-8, 6e-14
MARGIN = 10.0


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_sparse_grad_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse_grad.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_cov_pair_grad", "cimrgp_cov_pair_grad_scratch_bytes", "cimrgp_sparse_grad_combine",
                     "cimrgp_sparse_grad_rows"]
    assert sorted(_lib.SPARSE_GRAD_SIGNATURES) == names
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SPARSE_GRAD_SIGNATURES[name][1], name
    assert '#include "cimrgp_sparse_grad.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    build = open(os.path.join(ROOT, "cimrgp_amd", "csrc", "build.sh")).read()
    # every header beside cimrgp.h is a dependency of every object: the build script takes them by pattern
    assert " sparse_grad;" in build and "for h in *.hpp ../../include/*.h" in build and '"$h" -nt "$f.o"' in build


def test_pair_grad_scratch_bytes_by_formula():
    lib = _lib.load()
    for na, nb, d in ((1, 1, 1), (255, 100, 2), (4097, 130, 3), (3001, 257, 8), (65536, 1024, 2), (262144, 1000, 2),
                      (1 << 24, 1 << 20, 8)):
        assert int(lib.cimrgp_cov_pair_grad_scratch_bytes(na, nb, d)) == sg.pair_scratch_bytes(na, nb, d), (na, nb, d)
    for bad in ((0, 16, 1), (16, 0, 1), ((1 << 24) + 1, 16, 1), (16, (1 << 20) + 1, 1), (16, 16, 0), (16, 16, 9)):
        assert int(lib.cimrgp_cov_pair_grad_scratch_bytes(*bad)) == 0, bad
    # the slice count depends on (na, nb) alone; it fills the machine where there are rows to cut
    assert sg.pair_slices(4097, 130)[0] == 17 and sg.pair_slices(3001, 257)[0] == 12 and sg.pair_slices(255, 100) == (1, 256)
    assert sg.pair_slices(65536, 1024) == (128, 512)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 1, 2, 3])
@pytest.mark.parametrize("d", [1, 2])
def test_the_two_oracle_forms_agree_and_match_central_differences(d, cov, mode):
    """The NumPy chain, torch FP64 CPU autograd of the Woodbury chain and central differences (step 1e-5) of
    sparse_numpy.woodbury, at the shapes and parameters of the issue and 10 x the agreement it reports.  Inputs:
    sparse_numpy.problem with the seed n + m + d + cov (the convention of tests/test_sparse_host.py), Z moved off the
    data by 0.05 N(0, 1).  The gradient w.r.t. Z is as ill-conditioned as K_uu: the RBF at d = 1 has its own level."""
    x, z, r = sg.problem(N, M, d, seed=N + M + d + cov, q=Q)
    lml, dtheta, dz, parts = sg.chain(x, z, r, cov, ELL, SF, NOISE, EPS, mode)
    la, ta, za = sg.autograd(x, z, r, cov, ELL, SF, NOISE, EPS, mode)
    lw = sn.woodbury(x, z, r, cov, ELL, SF, NOISE, EPS, mode)[0]
    central = sg.central_theta(x, z, r, cov, ELL, SF, NOISE, EPS, mode)
    zlevel = Z_LEVEL_RBF_1D if (cov == 0 and d == 1) else Z_LEVEL
    print("d %d cov %d mode %d: value %.1e / %.1e  theta %.1e  Z %.1e  central %.1e"
          % (d, cov, mode, abs(la - lw) / abs(lw), abs(lml - lw) / abs(lw), _rel(dtheta, ta), _rel(dz, za), _rel(central, ta)))
    assert abs(la - lw) <= MARGIN * VALUE_LEVEL * abs(lw) and abs(lml - lw) <= MARGIN * VALUE_LEVEL * abs(lw)
    assert _rel(dtheta, ta) <= MARGIN * THETA_LEVEL
    assert _rel(dz, za) <= MARGIN * zlevel
    assert _rel(central, ta) <= MARGIN * CENTRAL_LEVEL


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
def test_closed_form_of_the_variance_derivative(cov, mode):
    """1/2 tr M + sf sum t equals sum G_fu o K_fu + sum G_uu o (K_uu + eps sf I) + sf sum t: k is linear in sf, so both are
    d F / d log sf; they differ by the rounding of the two triangular solves behind G_fu and G_uu (cond(L_u)^2 ~ m / eps)."""
    x, z, r = sg.problem(N, M, 2, seed=N + M + 2 + cov, q=Q)
    _, dtheta, _, parts = sg.chain(x, z, r, cov, ELL, SF, NOISE, EPS, mode)
    print(parts["closed"], parts["pairwise"])
    assert dtheta[0] == parts["closed"]
    assert abs(parts["closed"] - parts["pairwise"]) <= 2.0 ** -53 * M / EPS * abs(parts["closed"])
    # M = A^T G_A, the definition the closed form of M restates
    assert _rel(parts["a"].T @ parts["ga"], parts["M"]) <= 1e-10


# ---- refusals --------------------------------------------------------------------------------------------------------
BASE = {
    'cimrgp_cov_pair_grad': [('dtype', 1), ('cov', 0), ('xa', 'P'), ('na', 600), ('xb', 'P'), ('nb', 100), ('d', 2), ('g', 'P'),
        ('ldg', 112), ('ell', 0.7), ('sf2', 1.3), ('scale', 1.0), ('accumulate', 0), ('sums', 'P'), ('db', 'P'), ('scratch', 'P'),
        ('scratch_bytes', 1 << 20), ('stream', None)],
    'cimrgp_sparse_grad_rows': [('dtype', 1), ('v', 'P'), ('n', 600), ('m', 100), ('ldv', 112), ('gamma', 'P'), ('r', 'P'),
        ('w', 'P'), ('q', 2), ('mode', 0), ('noise', 0.01), ('beta', 'P'), ('t', 'P'), ('sums', 'P'), ('stream', None)],
    'cimrgp_sparse_grad_combine': [('dtype', 1), ('a', 'P'), ('lda', 112), ('y', 'P'), ('ldy', 112), ('n', 600), ('m', 100),
        ('beta', 'P'), ('b', 'P'), ('w', 'P'), ('t', 'P'), ('q', 2), ('stream', None)],
}

ROWS = [
    ('cimrgp_cov_pair_grad', {'dtype': 7}, -1, 'cimrgp_cov_pair_grad: unknown dtype'),
    ('cimrgp_cov_pair_grad', {'cov': 4}, -1, 'cimrgp_cov_pair_grad: unknown covariance'),
    ('cimrgp_cov_pair_grad', {'cov': -1}, -1, 'cimrgp_cov_pair_grad: unknown covariance'),
    ('cimrgp_cov_pair_grad', {'xa': None}, -1, 'cimrgp_cov_pair_grad: null pointer'),
    ('cimrgp_cov_pair_grad', {'xb': None}, -1, 'cimrgp_cov_pair_grad: null pointer'),
    ('cimrgp_cov_pair_grad', {'g': None}, -1, 'cimrgp_cov_pair_grad: null pointer'),
    ('cimrgp_cov_pair_grad', {'scratch': None}, -1, 'cimrgp_cov_pair_grad: null pointer'),
    ('cimrgp_cov_pair_grad', {'na': 0}, -1, 'cimrgp_cov_pair_grad: na must be in [1, 16777216]'),
    ('cimrgp_cov_pair_grad', {'na': (1 << 24) + 1}, -1, 'cimrgp_cov_pair_grad: na must be in [1, 16777216]'),
    ('cimrgp_cov_pair_grad', {'nb': 0}, -1, 'cimrgp_cov_pair_grad: nb must be in [1, 1048576]'),
    ('cimrgp_cov_pair_grad', {'nb': (1 << 20) + 1, 'ldg': 1 << 21}, -1, 'cimrgp_cov_pair_grad: nb must be in [1, 1048576]'),
    ('cimrgp_cov_pair_grad', {'d': 0}, -1, 'cimrgp_cov_pair_grad: input dimension must be in [1, 8]'),
    ('cimrgp_cov_pair_grad', {'d': 9}, -1, 'cimrgp_cov_pair_grad: input dimension must be in [1, 8]'),
    ('cimrgp_cov_pair_grad', {'ldg': 99}, -1, 'cimrgp_cov_pair_grad: leading dimension too small'),
    ('cimrgp_cov_pair_grad', {'ell': 0.0}, -1, 'cimrgp_cov_pair_grad: kernel parameters must be positive'),
    ('cimrgp_cov_pair_grad', {'sf2': -1.0}, -1, 'cimrgp_cov_pair_grad: kernel parameters must be positive'),
    ('cimrgp_cov_pair_grad', {'scratch': 'P+4'}, -1, 'cimrgp_cov_pair_grad: scratch must be 8-byte aligned'),
    ('cimrgp_cov_pair_grad', {'scratch_bytes': 6191}, -1, 'cimrgp_cov_pair_grad: scratch too small'),
    ('cimrgp_cov_pair_grad', {'dtype': 7, 'cov': 9, 'xa': None, 'na': 0, 'd': 0}, -1, 'cimrgp_cov_pair_grad: unknown dtype'),
    ('cimrgp_cov_pair_grad', {'sums': None, 'db': None, 'scratch_bytes': 0}, -1, 'cimrgp_cov_pair_grad: scratch too small'),
    ('cimrgp_sparse_grad_rows', {'dtype': 7}, -1, 'cimrgp_sparse_grad_rows: unknown dtype'),
    ('cimrgp_sparse_grad_rows', {'v': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'gamma': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'r': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'w': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'beta': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'t': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'sums': None}, -1, 'cimrgp_sparse_grad_rows: null pointer'),
    ('cimrgp_sparse_grad_rows', {'n': 0}, -1, 'cimrgp_sparse_grad_rows: bad dimensions'),
    ('cimrgp_sparse_grad_rows', {'n': 1 << 31}, -1, 'cimrgp_sparse_grad_rows: bad dimensions'),
    ('cimrgp_sparse_grad_rows', {'m': 0}, -1, 'cimrgp_sparse_grad_rows: bad dimensions'),
    ('cimrgp_sparse_grad_rows', {'ldv': 99}, -1, 'cimrgp_sparse_grad_rows: bad dimensions'),
    ('cimrgp_sparse_grad_rows', {'q': 0}, -1, 'cimrgp_sparse_grad_rows: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_grad_rows', {'q': 9}, -1, 'cimrgp_sparse_grad_rows: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_grad_rows', {'mode': 2}, -1, 'cimrgp_sparse_grad_rows: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_grad_rows', {'noise': 0.0}, -1, 'cimrgp_sparse_grad_rows: noise must be positive'),
    ('cimrgp_sparse_grad_rows', {'dtype': 7, 'v': None, 'n': 0, 'q': 0, 'mode': 2, 'noise': 0.0}, -1,
     'cimrgp_sparse_grad_rows: unknown dtype'),
    ('cimrgp_sparse_grad_combine', {'dtype': 7}, -1, 'cimrgp_sparse_grad_combine: unknown dtype'),
    ('cimrgp_sparse_grad_combine', {'a': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'y': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'beta': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'b': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'w': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'t': None}, -1, 'cimrgp_sparse_grad_combine: null pointer'),
    ('cimrgp_sparse_grad_combine', {'n': 0}, -1, 'cimrgp_sparse_grad_combine: bad dimensions'),
    ('cimrgp_sparse_grad_combine', {'n': 1 << 31}, -1, 'cimrgp_sparse_grad_combine: bad dimensions'),
    ('cimrgp_sparse_grad_combine', {'m': 0}, -1, 'cimrgp_sparse_grad_combine: bad dimensions'),
    ('cimrgp_sparse_grad_combine', {'lda': 99}, -1, 'cimrgp_sparse_grad_combine: bad dimensions'),
    ('cimrgp_sparse_grad_combine', {'ldy': 99}, -1, 'cimrgp_sparse_grad_combine: bad dimensions'),
    ('cimrgp_sparse_grad_combine', {'q': 0}, -1, 'cimrgp_sparse_grad_combine: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_grad_combine', {'q': 9}, -1, 'cimrgp_sparse_grad_combine: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_grad_combine', {'dtype': 7, 'a': None, 'n': 0, 'q': 0}, -1, 'cimrgp_sparse_grad_combine: unknown dtype'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [
    ('cimrgp_cov_pair_grad', {'sums': None, 'db': None}),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+4": p + 4}


def test_every_sparse_grad_entry_point_that_can_refuse_has_rows():
    assert set(BASE) | {"cimrgp_cov_pair_grad_scratch_bytes"} == set(_lib.SPARSE_GRAD_SIGNATURES)
    assert {row[0] for row in ROWS} == set(BASE)
    for name, base in BASE.items():
        assert len(base) == len(_lib.SPARSE_GRAD_SIGNATURES[name][1]), name
    # the scratch the base row of the pair contraction passes is enough, and one byte less than needed is refused
    assert sg.pair_scratch_bytes(600, 100, 2) == 6192


@pytest.mark.parametrize("name", sorted(BASE))
def test_sparse_grad_refusals_status_and_text(name):
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE[name]]
    for _, broken, status, text in [row for row in ROWS if row[0] == name]:
        assert broken and set(broken) <= set(keys), broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_sparse_grad_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name, broken in NO_WORK:
        assert getattr(lib, name)(*_args(name, broken, stand_in)) == 0, (name, broken)


# ---- the plugin's keywords -------------------------------------------------------------------------------------------
def test_keyword_validation():
    from cimrgp_amd import SGP_FITC, SparseGP, SparseGP_RBF
    for cls in (SparseGP, SGP_FITC, SparseGP_RBF):
        g = cls()
        assert (g.jac, g.optimize_inducing, g.optimize, g.inducing_inputs) == ('2-point', False, False, None)
        with pytest.raises(ValueError, match="optimize_inducing"):
            cls(optimize_inducing=True)
        with pytest.raises(ValueError, match="optimize_inducing"):
            cls(optimize=True, optimize_inducing=True)
        with pytest.raises(ValueError, match="optimize_inducing"):
            cls(jac='analytic', optimize_inducing=True)
        with pytest.raises(ValueError, match="jac"):
            cls(jac='3-point')
        with pytest.raises(ValueError, match="jac"):
            cls(jac=None)
        g = cls(optimize=True, jac='analytic', optimize_inducing=True)
        assert (g.jac, g.optimize_inducing) == ('analytic', True)
    g = SGP_FITC()
    g.preprocess = False
    with pytest.raises(RuntimeError, match="fit"):
        g.log_marginal_likelihood_grad()
