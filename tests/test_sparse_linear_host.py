"""CPU tests of the sparse GP's linear term (include/cimrgp_sparse_linear.h; DESIGN.md, "A linear term for the sparse GP"):
the header's symbols, every refusal of its four entry points that precedes a HIP call as a literal table, the scratch
formula, the two forms of the oracle tests/sparse_linear_numpy.py against each other, against tests/sparse_numpy.py at v = 0
and against central differences, the keyword rules of ``SparseGP_RBFLinear`` and ``SparseBlock(linear=)``, the TypeError
refusals of the queries that are not built, and the ``Hyper`` helpers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cimrgp_amd as ca
from cimrgp_amd import Hyper, _lib
from cimrgp_amd.Sparse import SparseBlock

import sparse_ard_numpy as sa
import sparse_grad_numpy as sg
import sparse_linear_numpy as sl
import sparse_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, M, Q = 300, 40, 2
ELLS = (0.7, 1.3, 2.1)
LIN = (0.5, 0.2, 0.35)
SF, NOISE, EPS = 1.3, 0.02, 1e-6
#: the largest relative gap between the oracle's gradient (autograd of the dense definition) and central differences of its
#: Woodbury form over the 32 cases below, as test_oracle_gradient_against_central_differences prints it (DESIGN.md records
#: the figure: 4.72e-7, a dZ entry of the RBF at d = 2, where the differences themselves carry rounding noise of that size);
#: asserted at 10 x, and 10 x this figure is the bound of the GPU test of the plugin's gradient against central differences
CENTRAL_LEVEL = 4.8e-7
MARGIN = 10.0

NAMES = ["cimrgp_cov_cross_lin", "cimrgp_cov_gram_lin", "cimrgp_cov_pair_grad_lin", "cimrgp_cov_pair_grad_lin_scratch_bytes",
         "cimrgp_sparse_lambda_kd"]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_sparse_linear_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse_linear.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == NAMES == sorted(_lib.SPARSE_LINEAR_SIGNATURES)
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SPARSE_LINEAR_SIGNATURES[name][1], name
        assert getattr(lib, name).restype == _lib.SPARSE_LINEAR_SIGNATURES[name][0], name
    assert _lib.HEADERS["cimrgp_sparse_linear.h"] is _lib.SPARSE_LINEAR_SIGNATURES
    assert '#include "cimrgp_sparse_linear.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    # each is its twin with the new arguments in place
    sig = _lib.signatures()
    for name, twin, more in (("cimrgp_cov_gram_lin", "cimrgp_cov_gram", 1), ("cimrgp_cov_cross_lin", "cimrgp_cov_cross", 1),
                             ("cimrgp_sparse_lambda_kd", "cimrgp_sparse_lambda", 0), ("cimrgp_cov_pair_grad_lin", "cimrgp_cov_pair_grad", 3),
                             ("cimrgp_cov_pair_grad_lin_scratch_bytes", "cimrgp_cov_pair_grad_scratch_bytes", 1)):
        assert len(sig[name][1]) == len(sig[twin][1]) + more, name
    assert {name for name in BASE} | {"cimrgp_cov_pair_grad_lin_scratch_bytes"} == set(NAMES)
    assert ca.SparseGP_RBFLinear.__name__ in ca.__all__


def test_pair_grad_lin_scratch_bytes_by_formula():
    lib = _lib.load()
    fn = lib.cimrgp_cov_pair_grad_lin_scratch_bytes
    assert sl.pair_scratch_bytes(600, 100, 2, False) == 12336 and sl.pair_scratch_bytes(600, 100, 2, True) == 12360
    for na, nb, d in ((65536, 1024, 2), (4097, 130, 3), (1, 1, 1), (255, 100, 2), (3001, 257, 8), (1 << 24, 1 << 20, 8)):
        for ard in (0, 1):
            assert int(fn(na, nb, d, ard)) == sl.pair_scratch_bytes(na, nb, d, bool(ard)), (na, nb, d, ard)
        # the twin's plus the second partial array
        assert int(fn(na, nb, d, 0)) - int(lib.cimrgp_cov_pair_grad_scratch_bytes(na, nb, d)) \
            == int(fn(na, nb, d, 1)) - int(lib.cimrgp_cov_pair_grad_ard_scratch_bytes(na, nb, d)) \
            == 8 * sg.pair_slices(na, nb)[0] * ((nb + 127) // 128) * 128 * d
    for bad in ((0, 16, 1), (16, 0, 1), ((1 << 24) + 1, 16, 1), (16, (1 << 20) + 1, 1), (16, 16, 0), (16, 16, 9)):
        assert int(fn(*bad, 0)) == 0 and int(fn(*bad, 1)) == 0, bad


# ---- refusals --------------------------------------------------------------------------------------------------------
BASE = {
    'cimrgp_cov_gram_lin': [('dtype', 1), ('cov', 0), ('x', 'P'), ('n', 100), ('d', 2), ('ell', 0.7), ('sf2', 1.3), ('lin', 'P'),
        ('diag_add', 0.0), ('k', 'P'), ('ldk', 112), ('lower_only', 0), ('stream', None)],
    'cimrgp_cov_cross_lin': [('dtype', 1), ('cov', 0), ('xa', 'P'), ('na', 50), ('xb', 'P'), ('nb', 100), ('d', 2), ('ell', 0.7),
        ('sf2', 1.3), ('lin', 'P'), ('kab', 'P'), ('ld', 112), ('stream', None)],
    'cimrgp_sparse_lambda_kd': [('dtype', 1), ('a', 'P'), ('n', 600), ('m', 100), ('lda', 112), ('kdiag', 'P'), ('noise', 0.05),
        ('mode', 0), ('lam', 'P'), ('w', 'P'), ('sums', 'P'), ('stream', None)],
    'cimrgp_cov_pair_grad_lin': [('dtype', 1), ('cov', 0), ('xa', 'P'), ('na', 600), ('xb', 'P'), ('nb', 100), ('d', 2), ('g', 'P'),
        ('ldg', 112), ('ell', 0.7), ('sf2', 1.3), ('ard', 0), ('lin', 'P'), ('scale', 1.0), ('accumulate', 0), ('sums', 'P'),
        ('lsums', 'P'), ('db', 'P'), ('scratch', 'P'), ('scratch_bytes', 1 << 20), ('stream', None)],
}

ROWS = [
    ('cimrgp_cov_gram_lin', {'x': None}, -1, 'cimrgp_cov_gram_lin: null pointer'),
    ('cimrgp_cov_gram_lin', {'k': None}, -1, 'cimrgp_cov_gram_lin: null pointer'),
    ('cimrgp_cov_gram_lin', {'lin': None}, -1, 'cimrgp_cov_gram_lin: null pointer (lin)'),
    ('cimrgp_cov_gram_lin', {'cov': 4}, -1, 'cimrgp_cov_gram_lin: unknown covariance'),
    ('cimrgp_cov_gram_lin', {'cov': -1}, -1, 'cimrgp_cov_gram_lin: unknown covariance'),
    ('cimrgp_cov_gram_lin', {'n': -1}, -1, 'cimrgp_cov_gram_lin: negative size'),
    ('cimrgp_cov_gram_lin', {'dtype': 7}, -1, 'cimrgp_cov_gram_lin: unknown dtype'),
    ('cimrgp_cov_gram_lin', {'d': 0}, -1, 'cimrgp_cov_gram_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_gram_lin', {'d': 9}, -1, 'cimrgp_cov_gram_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_gram_lin', {'ell': 0.0}, -1, 'cimrgp_cov_gram_lin: length-scale must be positive'),
    ('cimrgp_cov_gram_lin', {'ldk': 99}, -1, 'cimrgp_cov_gram_lin: leading dimension smaller than the number of columns'),
    ('cimrgp_cov_gram_lin', {'n': 1 << 30, 'ldk': 1 << 30}, -1, 'cimrgp_cov_gram_lin: matrix too large'),
    ('cimrgp_cov_gram_lin', {'n': (1 << 30) - 1, 'ldk': 1 << 30}, -1, 'cimrgp_cov_gram_lin: grid too large'),
    ('cimrgp_cov_gram_lin', {'n': (1 << 30) - 1, 'ldk': 1 << 30, 'lower_only': 1}, -1, 'cimrgp_cov_gram_lin: grid too large'),
    ('cimrgp_cov_gram_lin', {'x': None, 'lin': None, 'cov': 9, 'dtype': 7}, -1, 'cimrgp_cov_gram_lin: null pointer'),
    ('cimrgp_cov_gram_lin', {'lin': None, 'cov': 9, 'dtype': 7, 'd': 0}, -1, 'cimrgp_cov_gram_lin: null pointer (lin)'),
    ('cimrgp_cov_cross_lin', {'xa': None}, -1, 'cimrgp_cov_cross_lin: null pointer'),
    ('cimrgp_cov_cross_lin', {'xb': None}, -1, 'cimrgp_cov_cross_lin: null pointer'),
    ('cimrgp_cov_cross_lin', {'kab': None}, -1, 'cimrgp_cov_cross_lin: null pointer'),
    ('cimrgp_cov_cross_lin', {'lin': None}, -1, 'cimrgp_cov_cross_lin: null pointer (lin)'),
    ('cimrgp_cov_cross_lin', {'cov': 4}, -1, 'cimrgp_cov_cross_lin: unknown covariance'),
    ('cimrgp_cov_cross_lin', {'na': -1}, -1, 'cimrgp_cov_cross_lin: negative size'),
    ('cimrgp_cov_cross_lin', {'nb': -1}, -1, 'cimrgp_cov_cross_lin: negative size'),
    ('cimrgp_cov_cross_lin', {'dtype': 7}, -1, 'cimrgp_cov_cross_lin: unknown dtype'),
    ('cimrgp_cov_cross_lin', {'d': 0}, -1, 'cimrgp_cov_cross_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_cross_lin', {'d': 9}, -1, 'cimrgp_cov_cross_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_cross_lin', {'ell': -1.0}, -1, 'cimrgp_cov_cross_lin: length-scale must be positive'),
    ('cimrgp_cov_cross_lin', {'ld': 99}, -1, 'cimrgp_cov_cross_lin: leading dimension smaller than the number of columns'),
    ('cimrgp_cov_cross_lin', {'na': 1 << 30}, -1, 'cimrgp_cov_cross_lin: matrix too large'),
    ('cimrgp_cov_cross_lin', {'na': (1 << 30) - 1, 'nb': (1 << 30) - 1, 'ld': 1 << 30}, -1, 'cimrgp_cov_cross_lin: grid too large'),
    ('cimrgp_cov_cross_lin', {'lin': None, 'cov': 9, 'na': -1}, -1, 'cimrgp_cov_cross_lin: null pointer (lin)'),
    ('cimrgp_sparse_lambda_kd', {'dtype': 7}, -1, 'cimrgp_sparse_lambda_kd: unknown dtype'),
    ('cimrgp_sparse_lambda_kd', {'a': None}, -1, 'cimrgp_sparse_lambda_kd: null pointer'),
    ('cimrgp_sparse_lambda_kd', {'lam': None}, -1, 'cimrgp_sparse_lambda_kd: null pointer'),
    ('cimrgp_sparse_lambda_kd', {'w': None}, -1, 'cimrgp_sparse_lambda_kd: null pointer'),
    ('cimrgp_sparse_lambda_kd', {'sums': None}, -1, 'cimrgp_sparse_lambda_kd: null pointer'),
    ('cimrgp_sparse_lambda_kd', {'kdiag': None}, -1, 'cimrgp_sparse_lambda_kd: null pointer (kdiag)'),
    ('cimrgp_sparse_lambda_kd', {'n': 0}, -1, 'cimrgp_sparse_lambda_kd: bad dimensions'),
    ('cimrgp_sparse_lambda_kd', {'n': 1 << 31}, -1, 'cimrgp_sparse_lambda_kd: bad dimensions'),
    ('cimrgp_sparse_lambda_kd', {'m': 0}, -1, 'cimrgp_sparse_lambda_kd: bad dimensions'),
    ('cimrgp_sparse_lambda_kd', {'lda': 99}, -1, 'cimrgp_sparse_lambda_kd: bad dimensions'),
    ('cimrgp_sparse_lambda_kd', {'mode': 2}, -1, 'cimrgp_sparse_lambda_kd: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda_kd', {'mode': -1}, -1, 'cimrgp_sparse_lambda_kd: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda_kd', {'dtype': 7, 'a': None, 'kdiag': None, 'n': 0, 'mode': 2}, -1, 'cimrgp_sparse_lambda_kd: unknown dtype'),
    ('cimrgp_sparse_lambda_kd', {'a': None, 'kdiag': None, 'n': 0}, -1, 'cimrgp_sparse_lambda_kd: null pointer'),
    ('cimrgp_cov_pair_grad_lin', {'dtype': 7}, -1, 'cimrgp_cov_pair_grad_lin: unknown dtype'),
    ('cimrgp_cov_pair_grad_lin', {'cov': 4}, -1, 'cimrgp_cov_pair_grad_lin: unknown covariance'),
    ('cimrgp_cov_pair_grad_lin', {'cov': -1}, -1, 'cimrgp_cov_pair_grad_lin: unknown covariance'),
    ('cimrgp_cov_pair_grad_lin', {'xa': None}, -1, 'cimrgp_cov_pair_grad_lin: null pointer'),
    ('cimrgp_cov_pair_grad_lin', {'xb': None}, -1, 'cimrgp_cov_pair_grad_lin: null pointer'),
    ('cimrgp_cov_pair_grad_lin', {'g': None}, -1, 'cimrgp_cov_pair_grad_lin: null pointer'),
    ('cimrgp_cov_pair_grad_lin', {'scratch': None}, -1, 'cimrgp_cov_pair_grad_lin: null pointer'),
    ('cimrgp_cov_pair_grad_lin', {'lin': None}, -1, 'cimrgp_cov_pair_grad_lin: null pointer (lin)'),
    ('cimrgp_cov_pair_grad_lin', {'na': 0}, -1, 'cimrgp_cov_pair_grad_lin: na must be in [1, 16777216]'),
    ('cimrgp_cov_pair_grad_lin', {'na': (1 << 24) + 1}, -1, 'cimrgp_cov_pair_grad_lin: na must be in [1, 16777216]'),
    ('cimrgp_cov_pair_grad_lin', {'nb': 0}, -1, 'cimrgp_cov_pair_grad_lin: nb must be in [1, 1048576]'),
    ('cimrgp_cov_pair_grad_lin', {'nb': (1 << 20) + 1, 'ldg': 1 << 21}, -1, 'cimrgp_cov_pair_grad_lin: nb must be in [1, 1048576]'),
    ('cimrgp_cov_pair_grad_lin', {'d': 0}, -1, 'cimrgp_cov_pair_grad_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_pair_grad_lin', {'d': 9}, -1, 'cimrgp_cov_pair_grad_lin: input dimension must be in [1, 8]'),
    ('cimrgp_cov_pair_grad_lin', {'ldg': 99}, -1, 'cimrgp_cov_pair_grad_lin: leading dimension too small'),
    ('cimrgp_cov_pair_grad_lin', {'ell': 0.0}, -1, 'cimrgp_cov_pair_grad_lin: kernel parameters must be positive'),
    ('cimrgp_cov_pair_grad_lin', {'sf2': -1.0}, -1, 'cimrgp_cov_pair_grad_lin: kernel parameters must be positive'),
    ('cimrgp_cov_pair_grad_lin', {'scratch': 'P+4'}, -1, 'cimrgp_cov_pair_grad_lin: scratch must be 8-byte aligned'),
    ('cimrgp_cov_pair_grad_lin', {'scratch_bytes': 12335}, -1, 'cimrgp_cov_pair_grad_lin: scratch too small'),
    # what is enough without ARD (12336 bytes) is not enough with it, and the twins' sizes are not enough at all
    ('cimrgp_cov_pair_grad_lin', {'ard': 1, 'scratch_bytes': 12336}, -1, 'cimrgp_cov_pair_grad_lin: scratch too small'),
    ('cimrgp_cov_pair_grad_lin', {'scratch_bytes': 6192}, -1, 'cimrgp_cov_pair_grad_lin: scratch too small'),
    ('cimrgp_cov_pair_grad_lin', {'ard': 1, 'scratch_bytes': 6216}, -1, 'cimrgp_cov_pair_grad_lin: scratch too small'),
    ('cimrgp_cov_pair_grad_lin', {'dtype': 7, 'cov': 9, 'xa': None, 'lin': None, 'na': 0, 'd': 0}, -1,
     'cimrgp_cov_pair_grad_lin: unknown dtype'),
    ('cimrgp_cov_pair_grad_lin', {'dtype': 7, 'cov': 9, 'xa': None, 'na': 0, 'd': 0}, -1, 'cimrgp_cov_pair_grad_lin: unknown dtype'),
    ('cimrgp_cov_pair_grad_lin', {'sums': None, 'lsums': None, 'db': None, 'scratch_bytes': 0}, -1,
     'cimrgp_cov_pair_grad_lin: scratch too small'),
    # the twin's outputs both NULL: lsums is still wanted, so the scratch is still checked and needed
    ('cimrgp_cov_pair_grad_lin', {'sums': None, 'db': None, 'scratch_bytes': 0}, -1, 'cimrgp_cov_pair_grad_lin: scratch too small'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [
    ('cimrgp_cov_gram_lin', {'n': 0}),
    ('cimrgp_cov_cross_lin', {'na': 0}),
    ('cimrgp_cov_cross_lin', {'nb': 0}),
    ('cimrgp_cov_pair_grad_lin', {'sums': None, 'lsums': None, 'db': None}),
    ('cimrgp_cov_pair_grad_lin', {'sums': None, 'lsums': None, 'db': None, 'scratch_bytes': 12336}),
    ('cimrgp_cov_pair_grad_lin', {'sums': None, 'lsums': None, 'db': None, 'ard': 1, 'scratch_bytes': 12360}),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+4": p + 4}


@pytest.mark.parametrize("name", sorted(BASE))
def test_sparse_linear_refusals_status_and_text(name):
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE[name]]
    assert len(keys) == len(_lib.SPARSE_LINEAR_SIGNATURES[name][1])
    rows = [row for row in ROWS if row[0] == name]
    assert rows
    for _, broken, status, text in rows:
        assert broken and set(broken) <= set(keys), broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_sparse_linear_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name, broken in NO_WORK:
        assert getattr(lib, name)(*_args(name, broken, stand_in)) == 0, (name, broken)


def test_the_refusal_rows_hold_the_twins_rows_under_the_new_names():
    """Nothing the twins refuse is let through: every row of the pair contraction's and of the lambda pass's tables is here."""
    import test_sparse_grad_host as grad_twin
    import test_sparse_layer_refusals_host as layer_twin
    mine = {(name, tuple(sorted(b.items())), st, tx) for name, b, st, tx in ROWS}
    for name, broken, status, text in grad_twin.ROWS:
        if name != 'cimrgp_cov_pair_grad':
            continue
        if broken == {'scratch_bytes': 6191}:
            broken = {'scratch_bytes': 12335}
        key = ('cimrgp_cov_pair_grad_lin', tuple(sorted(broken.items())), status, text.replace('cimrgp_cov_pair_grad', 'cimrgp_cov_pair_grad_lin'))
        assert key in mine, broken
    for name, broken, status, text in layer_twin.ROWS:
        if name != 'cimrgp_sparse_lambda_dev':
            continue
        broken = {('kdiag' if k == 'noise' else k): v for k, v in broken.items()}
        key = ('cimrgp_sparse_lambda_kd', tuple(sorted(broken.items())), status,
               text.replace('cimrgp_sparse_lambda_dev', 'cimrgp_sparse_lambda_kd').replace('(noise)', '(kdiag)'))
        assert key in mine, broken


# ---- the oracle ----------------------------------------------------------------------------------------------------
def _ell(d, ard):
    return np.array(ELLS[:d]) if ard else 0.9


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("cov", (0, 1, 2, 3))
def test_oracle_forms_agree(cov, mode):
    for d, ard in ((2, True), (3, False)):
        x, z, r, xs = sn.problem(N, M, d, 7 + d)
        lin = np.array(LIN[:d])
        for include_noise in (False, True):
            w = sl.woodbury(x, z, r, cov, _ell(d, ard), SF, NOISE, EPS, mode, lin, xs, include_noise)
            dn = sl.dense(x, z, r, cov, _ell(d, ard), SF, NOISE, EPS, mode, lin, xs, include_noise)
            assert abs(w[0] - dn[0]) <= 1e-9 * abs(dn[0])
            assert _rel(w[1], dn[1]) < 1e-8 and _rel(w[2], dn[2]) < 1e-8
        # the term is there: the same model without it predicts something else
        w0 = sl.woodbury(x, z, r, cov, _ell(d, ard), SF, NOISE, EPS, mode, np.zeros(d), xs)
        assert _rel(w0[2], w[2]) > 1e-3


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("cov", (0, 1, 2, 3))
def test_oracle_without_the_term_is_the_sparse_oracle_exactly(cov, mode):
    x, z, r, xs = sn.problem(N, M, 2, 11)
    for form, twin in ((sl.woodbury, sn.woodbury), (sl.dense, sn.dense)):
        got = form(x, z, r, cov, 0.9, SF, NOISE, EPS, mode, np.zeros(2), xs, True)
        want = twin(x, z, r, cov, 0.9, SF, NOISE, EPS, mode, xs, True)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_oracle_gradient_against_central_differences():
    """Autograd of the dense definition against central differences of the Woodbury form: n = 300, m = 40, d in {2, 3}, four
    covariances, FITC and VFE, ARD and isotropic.  The largest relative gap is printed; CENTRAL_LEVEL records it."""
    worst = 0.0
    for d in (2, 3):
        x, z, r = sg.problem(N, M, d, 20 + d)
        lin = np.array(LIN[:d])
        for cov in (0, 1, 2, 3):
            for mode in (0, 1):
                for ard in (True, False):
                    ell = _ell(d, ard)
                    lml, dth, dz = sl.grad_dense(x, z, r, cov, ell, SF, NOISE, EPS, mode, lin)
                    assert dth.shape == (2 + np.size(ell) + d,) and dz.shape == z.shape
                    _, wth, wz = sl.grad_woodbury(x, z, r, cov, ell, SF, NOISE, EPS, mode, lin)
                    assert _rel(wth, dth) < 1e-9 and _rel(wz, dz) < 1e-7     # the two forms of the gradient
                    assert abs(lml - sl.woodbury(x, z, r, cov, ell, SF, NOISE, EPS, mode, lin)[0]) <= 1e-9 * abs(lml)
                    cth, cz = sl.central(x, z, r, cov, ell, SF, NOISE, EPS, mode, lin, want_z_rows=(0, M // 2))
                    gz = np.array([dz[j, e] for (j, e) in cz])
                    gap = max(_rel(dth, cth), float(np.abs(gz - np.array(list(cz.values()))).max() / np.abs(dz).max()))
                    print("d %d cov %d mode %d ard %d: gap %.2e" % (d, cov, mode, ard, gap))
                    worst = max(worst, gap)
    print("largest relative gap to central differences: %.2e" % worst)
    assert worst <= MARGIN * CENTRAL_LEVEL
    assert worst >= CENTRAL_LEVEL / 100.0, "CENTRAL_LEVEL no longer describes the oracle; measure it again"


def test_oracle_gradient_of_the_linear_variances_is_not_zero_and_ell_free():
    """The term does not depend on the length-scales: at fixed v, changing l moves only the covariance part."""
    x, z, r = sg.problem(N, M, 2, 5)
    lin = np.array(LIN[:2])
    _, dth, _ = sl.grad_dense(x, z, r, 0, np.array(ELLS[:2]), SF, NOISE, EPS, 1, lin)
    assert np.abs(dth[-2:]).min() > 1e-3
    a = sl.ksum(x, z, 0, np.array(ELLS[:2]), SF, lin) - sl.ksum(x, z, 0, np.array(ELLS[:2]), SF, 0 * lin)
    b = sl.ksum(x, z, 0, np.array([3.0, 0.4]), SF, lin) - sl.ksum(x, z, 0, np.array([3.0, 0.4]), SF, 0 * lin)
    assert np.abs(a - b).max() < 1e-14 * np.abs(a).max() + 1e-15


def test_the_two_oracle_models_differ_on_the_trend_case():
    """The case of the GPU plugin test, on the CPU first: with a trend in the labels the RBF + Linear oracle extrapolates it
    at x0 = 2, the RBF-only oracle reverts towards the mean: a clear margin between the two errors."""
    x, y, target = sl.trend_problem(400, 0)
    mu, sd, ym, ys = x.mean(0), x.std(0), y.mean(0), y.std(0)
    xn, yn = (x - mu) / sd, (y - ym) / ys
    z = xn[np.random.RandomState(0).permutation(400)[:60]]
    xs = (np.array([[2.0]]) - mu) / sd
    noise = float(yn.var()) * 0.01
    with_term = sl.woodbury(xn, z, yn, 0, np.array([1.0]), 1.0, noise, 1e-6, 1, np.array([1.0]), xs)[1] * ys + ym
    without = sn.woodbury(xn, z, yn, 0, 1.0, 1.0, noise, 1e-6, 1, xs)[1] * ys + ym
    e_with, e_without = abs(float(with_term[0, 0]) - target(2.0)), abs(float(without[0, 0]) - target(2.0))
    print("error at x0 = 2: with the term %.3f, without %.3f" % (e_with, e_without))
    assert e_with < 0.5 * e_without and e_without - e_with > 0.5


# ---- the Python layer ----------------------------------------------------------------------------------------------
def test_hyper_helpers_round_trip_and_pack_theta_is_unchanged():
    assert np.array_equal(Hyper.pack_theta(1.3, 0.7, 0.02), np.log([1.3, 0.7, 0.02]))
    assert np.array_equal(Hyper.pack_theta(1.3, [0.7, 1.1], 0.02), np.log([1.3, 0.7, 1.1, 0.02]))
    assert list(inspect.signature(Hyper.pack_theta).parameters) == ['sf', 'ell', 'noise']
    assert list(inspect.signature(Hyper.unpack_theta).parameters) == ['theta', 'n_ell']
    lin = np.array([0.5, 0.2, 0.35])
    zflat = np.arange(6.0)
    for ell, n_ell in ((0.7, None), (np.array([0.7, 1.1, 2.0]), 3)):
        head = Hyper.pack_theta(1.3, ell, 0.02)
        theta = np.concatenate([Hyper.append_linear(head, lin), zflat])
        assert theta.shape[0] == head.shape[0] + 3 + 6 and np.array_equal(theta[:head.shape[0]], head)
        h, v, rest = Hyper.split_linear(theta, 3, n_ell)
        assert np.array_equal(h, head) and np.allclose(v, lin, rtol=1e-15) and np.array_equal(rest, zflat)
        e, sf, noise = Hyper.unpack_theta(theta, n_ell)
        assert np.allclose(e, ell) and np.isclose(sf, 1.3) and np.isclose(noise, 0.02)
        v[0] = 9.0                                       # a fresh array
        assert theta[head.shape[0]] == np.log(0.5)


def test_new_class_signature_and_the_pinned_ones():
    want = ['self', 'num_inducing', 'lengthscale', 'variance', 'linear_variance', 'nu', 'Z', 'seed', 'jitter', 'dtype', 'device',
            'optimize', 'max_iters', 'jac', 'optimize_inducing', 'ARD', 'approximation']
    sig = inspect.signature(ca.SparseGP_RBFLinear.__init__).parameters
    assert list(sig) == want
    defaults = dict(num_inducing=1000, lengthscale=1., variance=1., linear_variance=1., nu=None, Z=None, seed=0, jitter=1e-6, dtype='f64',
                    device=None, optimize=False, max_iters=200, jac='2-point', optimize_inducing=False, ARD=True, approximation='vfe')
    assert {k: p.default for k, p in sig.items() if k != 'self'} == defaults
    for cls in (ca.SparseGP, ca.SGP_FITC, ca.SparseGP_RBF):
        assert list(inspect.signature(cls.__init__).parameters)[-1] == 'ARD'
        assert cls(num_inducing=4).linear_variances is None
    gp = ca.SparseGP_RBFLinear(num_inducing=4)
    assert isinstance(gp, ca.SparseGP) and gp.ARD and gp.approximation == 'vfe' and gp.linear_variances is None


def test_new_class_keyword_validation():
    for bad in (0.0, -1.0, np.nan, np.inf, [0.5, 0.0], [0.5, -0.2], [0.5, np.nan], [], [[0.5, 0.2]]):
        with pytest.raises(ValueError, match='linear_variance'):
            ca.SparseGP_RBFLinear(linear_variance=bad)
    with pytest.raises(ValueError, match="optimize_inducing=True needs optimize=True and jac='analytic'"):
        ca.SparseGP_RBFLinear(optimize_inducing=True)
    with pytest.raises(ValueError, match="optimize_inducing=True needs optimize=True and jac='analytic'"):
        ca.SparseGP_RBFLinear(optimize=True, optimize_inducing=True)
    ca.SparseGP_RBFLinear(optimize=True, jac='analytic', optimize_inducing=True)
    with pytest.raises(ValueError, match='approximation'):
        ca.SparseGP_RBFLinear(approximation='exact')
    # a wrong length is refused at fit, before the device is asked for
    rng = np.random.default_rng(0)
    data = [rng.normal(size=(30, 2)), rng.normal(size=(30, 1))]
    with pytest.raises(ValueError, match='linear_variance has 3 entries, the inputs have 2 dimensions'):
        ca.SparseGP_RBFLinear(num_inducing=5, linear_variance=[0.5, 0.2, 0.1]).fit(data)


def test_queries_that_are_not_built_raise_type_error():
    gp = ca.SparseGP_RBFLinear(num_inducing=4)
    xs = np.zeros((3, 2))
    for call in (lambda: gp.predictive_gradients(xs), lambda: gp.leave_one_out(), lambda: gp.loo_log_predictive_density(),
                 lambda: gp.predict_with_covariance(xs), lambda: gp.posterior_samples_f(xs)):
        with pytest.raises(TypeError, match='not yet supported'):
            call()
    # the block's: refused before any device work (the tensors here are the host's)
    x, z = torch.zeros(8, 2, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64)
    blk = SparseBlock(x, z, ca.RBFKernel(l=1.0, sf=1.0, noise=0.1), 'vfe', lengthscales=[0.7, 1.3], linear=[0.5, 0.2])
    assert np.allclose(blk.cov.u, [0.5 * 0.49, 0.2 * 1.69]) and np.array_equal(blk.linear, [0.5, 0.2])
    assert blk.cov.lin.dtype == torch.float64 and np.array_equal(blk.cov.lin.numpy(), blk.cov.u)
    blk.gamma = torch.zeros(3, 1, dtype=torch.float64)   # as after a fit
    for call in (lambda: blk.predict_grad(x), lambda: blk.loo(x[:, :1]), lambda: blk.joint(x)):
        with pytest.raises(TypeError, match='with a linear term is not yet supported'):
            call()
    with pytest.raises(TypeError, match='has no linear term'):
        g = ca.SparseGP_RBF(num_inducing=4)
        g.block = blk
        g.log_marginal_likelihood(linear=[0.5, 0.2])


def test_sparse_block_linear_refusals():
    x, z = torch.zeros(8, 2, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64)
    k = ca.RBFKernel(l=1.0, sf=1.0, noise=0.1)
    for bad in ([0.5], [0.5, 0.2, 0.1], [0.5, 0.0], [0.5, -1.0], [0.5, np.nan], [[0.5, 0.2]]):
        with pytest.raises(ValueError, match='linear must be 2 positive variances'):
            SparseBlock(x, z, k, linear=bad)
    with pytest.raises(ValueError, match='not available to a model layer'):
        SparseBlock(x, z, k, device_noise=True, linear=[0.5, 0.2])
    plain = SparseBlock(x, z, k)
    assert plain.linear is None and plain.cov.lin is None and plain.cov.u is None        # no linear term, no weights
