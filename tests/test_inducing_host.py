"""Greedy inducing-point selection without a GPU: the refusals of cimrgp_pivoted_cholesky that come before any device work
(status and exact text, one broken argument at a time, in the manner of test_abi_refusals_host.py), the 'greedy' rule of
``SparseKernel``, the host-side argument checks of ``Inducing.select_inducing`` and the NumPy oracle itself."""
import ctypes

import numpy as np
import pytest

import inducing_numpy as inp
from cimrgp_amd import _lib
from cimrgp_amd.KernelClass import DenseMaternKernel, RBFKernel, SparseKernel

FN = 'cimrgp_pivoted_cholesky'
BASE = [('dtype', 1), ('cov', 0), ('x', 'P'), ('n', 600), ('d', 2), ('ell', 1.0), ('sf2', 1.0), ('lin', None), ('m', 40),
        ('floor', 0.0), ('pivots', 'P'), ('lt', 'P'), ('ldl', 608), ('diag', 'P'), ('trace', 'P'), ('rank', 'P'), ('scratch', 'P'),
        ('scratch_bytes', 1 << 20), ('stream', None)]

ROWS = [
    ({'dtype': 7}, 'unknown dtype'),
    ({'dtype': 0}, "FP32 is not built (the residual's cancellation needs FP64)"),
    ({'cov': 4}, 'unknown covariance'),
    ({'cov': -1}, 'unknown covariance'),
    ({'x': None}, 'null pointer'),
    ({'pivots': None}, 'null pointer'),
    ({'lt': None}, 'null pointer'),
    ({'diag': None}, 'null pointer'),
    ({'trace': None}, 'null pointer'),
    ({'rank': None}, 'null pointer'),
    ({'scratch': None}, 'null pointer'),
    ({'n': 0}, 'n must be in [1, 2^31)'),
    ({'n': 1 << 31, 'ldl': 1 << 31}, 'n must be in [1, 2^31)'),
    ({'m': 601}, 'm must be in [1, n]'),
    ({'m': 0}, 'm must be in [1, n]'),
    ({'d': 0}, 'input dimension must be in [1, 8]'),
    ({'d': 9}, 'input dimension must be in [1, 8]'),
    ({'ell': 0.0}, 'ell and sf2 must be positive'),
    ({'sf2': -1.0}, 'ell and sf2 must be positive'),
    ({'sf2': float('nan')}, 'ell and sf2 must be positive'),
    ({'floor': -1e-300}, 'floor must be finite and not negative'),
    ({'floor': float('nan')}, 'floor must be finite and not negative'),
    ({'floor': float('inf')}, 'floor must be finite and not negative'),
    ({'ldl': 599}, 'leading dimension too small'),
    ({'scratch': 'P+8'}, 'scratch must be 16-byte aligned'),
    ({'scratch_bytes': 64}, 'scratch too small'),
    # every argument broken at once: the first check speaks
    ({'dtype': 7, 'cov': 9, 'x': None, 'n': 0, 'm': 0, 'd': 0, 'ell': 0.0, 'floor': -1.0, 'ldl': 0, 'scratch_bytes': 0}, 'unknown dtype'),
]


def test_entry_points_are_registered_under_their_own_header():
    assert _lib.HEADERS['cimrgp_inducing.h'] is _lib.INDUCING_SIGNATURES
    assert set(_lib.INDUCING_SIGNATURES) == {FN, FN + '_scratch_bytes'}
    assert len(BASE) == len(_lib.INDUCING_SIGNATURES[FN][1])
    lib = _lib.load()
    assert hasattr(lib, FN) and hasattr(lib, FN + '_scratch_bytes')


@pytest.mark.parametrize('broken,text', ROWS, ids=[' '.join(sorted(b)) + ':' + t[:24] for b, t in ROWS])
def test_refusals_status_and_text(broken, text):
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    stand_in = {'P': p, 'P+8': p + 8}
    assert set(broken) <= {k for k, _ in BASE}
    args = [broken.get(k, v) for k, v in BASE]
    args = [stand_in.get(a, a) if isinstance(a, str) else a for a in args]
    rc = getattr(lib, FN)(*args)
    assert (rc, _lib.last_error()) == (-1, FN + ': ' + text)


def test_scratch_query():
    lib = _lib.load()
    q = lib.cimrgp_pivoted_cholesky_scratch_bytes
    up = lambda b: (b + 15) // 16 * 16
    for n, m in ((1, 1), (600, 40), (4097, 5), (65536, 1000)):
        rec = -(-n // _lib.PIVCHOL_ROWS)
        assert q(n, m) == up(8 * m) + up(4 * n) + 2 * up(8 * rec) + up(4 * rec) + 16
    for n, m in ((0, 0), (10, 11), (10, 0), (1 << 31, 5), (-1, 1)):
        assert q(n, m) == 0


# ---- SparseKernel(inducing='greedy') ---------------------------------------------------------------------------------------
def test_sparse_kernel_takes_the_greedy_rule_and_keeps_it():
    assert SparseKernel.INDUCING == ('stride', 'random', 'greedy')
    k = SparseKernel(RBFKernel(l=0.5), num_inducing=48, approximation='vfe', inducing='greedy', seed=5)
    assert k.inducing == 'greedy' and k.num_inducing == 48
    for other in (k.rewrap(DenseMaternKernel(nu=1.5, l=0.3)), k.with_noise(0.02), k.with_values(0.7, 1.2, 0.03),
                  k.with_values([0.7, 0.9], 1.2, 0.03)):
        assert isinstance(other, SparseKernel)
        assert (other.inducing, other.num_inducing, other.approximation, other.jitter, other.seed) == ('greedy', 48, 'vfe', k.jitter, 5)
    assert k.with_noise(0.02).noise == 0.02 and k.with_values(0.7, 1.2, 0.03).l == 0.7


def test_greedy_rows_need_data():
    k = SparseKernel(RBFKernel(l=0.5), num_inducing=8, inducing='greedy')
    with pytest.raises(TypeError, match=r'SparsePosterior\.inducing_rows'):
        k.inducing_rows(0, 0, 100)
    # the other rules are untouched
    assert SparseKernel(RBFKernel(), 4).inducing_rows(0, 0, 10).tolist() == [1, 3, 6, 8]
    r = SparseKernel(RBFKernel(), 4, inducing='random', seed=2).inducing_rows(1, 3, 10)
    assert r.tolist() == np.random.RandomState([2, 1, 3]).permutation(10)[:4].tolist()


@pytest.mark.parametrize('rule', ['kmeans', 'Greedy', '', None])
def test_other_rules_are_still_refused(rule):
    with pytest.raises(ValueError, match='inducing must be'):
        SparseKernel(RBFKernel(), inducing=rule)


def test_posterior_has_no_greedy_rows_before_a_fit():
    from cimrgp_amd.Sparse import SparsePosterior
    post = SparsePosterior(2, 1, SparseKernel(RBFKernel(l=0.5), 8, inducing='greedy'), 0, [20, 21])
    with pytest.raises(RuntimeError, match='no greedy rows yet'):
        post.inducing_rows(1)
    stride = SparsePosterior(2, 1, SparseKernel(RBFKernel(l=0.5), 8), 0, [20, 21])
    assert stride.inducing_rows(1).tolist() == SparseKernel(RBFKernel(), 8).inducing_rows(0, 1, 21).tolist()


# ---- select_inducing: refused before any device is asked for ---------------------------------------------------------------
@pytest.mark.parametrize('kwargs,text', [
    (dict(num_inducing=0), 'num_inducing must be at least 1'),
    (dict(dtype='f32'), "built for dtype 'f64' only"),
    (dict(dtype='f16'), "dtype must be 'f32' or 'f64'"),
    (dict(X=np.zeros(5)), 'X must be an n x d matrix'),
    (dict(X=np.full((5, 2), np.nan)), 'X must be finite'),
    (dict(lengthscale=-1.0), 'lengthscale must be positive'),
    (dict(lengthscale=[0.5, 0.5]), 'needs ARD=True'),
    (dict(lengthscale=[0.5, 0.5, 0.5], ARD=True), 'lengthscale has 3 entries'),
    (dict(variance=0.0), 'variance must be a positive number'),
    (dict(linear_variance=[1.0, -1.0]), 'linear_variance must be positive'),
    (dict(linear_variance=[1.0, 1.0, 1.0]), 'linear_variance has 3 entries'),
    (dict(tol=-0.1), 'tol must not be negative'),
    (dict(nu=2.0), 'nu must be 0.5, 1.5 or 2.5'),
])
def test_select_inducing_argument_checks(kwargs, text):
    from cimrgp_amd.Inducing import select_inducing
    args = dict(X=np.random.default_rng(0).normal(size=(20, 2)), num_inducing=5)
    args.update(kwargs)
    with pytest.raises(ValueError) as err:
        select_inducing(**args)
    assert text in str(err.value)


def test_greedy_rows_argument_checks():
    import torch
    from cimrgp_amd.Inducing import greedy_rows
    x = torch.zeros(6, 2, dtype=torch.float64)
    with pytest.raises(TypeError, match='RBFKernel or a DenseMaternKernel'):
        greedy_rows(x, 3, SparseKernel(RBFKernel()))
    with pytest.raises(ValueError, match='float64'):
        greedy_rows(x.float(), 3, RBFKernel())
    with pytest.raises(ValueError, match='num_inducing'):
        greedy_rows(x, 0, RBFKernel())
    with pytest.raises(ValueError, match='floor must not be negative'):
        greedy_rows(x, 3, RBFKernel(), floor=float('nan'))
    with pytest.raises(ValueError, match='lengthscales beside'):
        greedy_rows(x, 3, RBFKernel(l=[1.0, 2.0]), lengthscales=[1.0, 2.0])


# ---- the oracle itself ------------------------------------------------------------------------------------------------------
def _problem(n, d, seed):
    return np.random.default_rng(seed).uniform(size=(n, d))


def test_oracle_full_rank_reproduces_the_permuted_matrix():
    x = _problem(60, 2, 1)
    for ft, tol in ((np.float64, 1e-12), (inp.LD, 1e-15)):
        o = inp.pivoted_cholesky(x, 60, inp.COV_MATERN12, 0.5, 1.3, ft=ft)
        p = o['pivots']
        assert sorted(p.tolist()) == list(range(60)) and o['rank'] == 60
        k = inp.cov_matrix(x, x, inp.COV_MATERN12, 0.5, 1.3, ft=ft)
        l = o['lt'].T[p]                       # rows in pivot order: lower triangular up to rounding
        assert float(np.abs(np.triu(l, 1)).max()) <= tol
        assert float(np.abs(l @ l.T - k[np.ix_(p, p)]).max()) <= tol
        assert (o['diag'] == -1).all() and float(o['trace'][-1]) == 0.0


def test_oracle_prefix_property_and_first_pivot():
    x = _problem(120, 3, 2)
    a = inp.pivoted_cholesky(x, 40, inp.COV_RBF, 0.5, 1.3)
    b = inp.pivoted_cholesky(x, 17, inp.COV_RBF, 0.5, 1.3)
    assert a['pivots'][0] == 0                  # an exact tie of a stationary kernel: the lowest row
    assert (a['pivots'][:17] == b['pivots']).all()
    assert a['trace'][:18].tobytes() == b['trace'].tobytes() and a['lt'][:17].tobytes() == b['lt'].tobytes()
    lin = inp.pivoted_cholesky(x, 5, inp.COV_RBF, 0.5, 1.3, lin=[0.5, 0.2, 0.1])
    assert lin['pivots'][0] == int(np.argmax((x * x * [0.5, 0.2, 0.1]).sum(axis=1)))


def test_oracle_trace_is_the_nystrom_slack():
    x = _problem(90, 2, 3)
    for cov, lin in ((inp.COV_RBF, None), (inp.COV_MATERN32, None), (inp.COV_RBF, [0.5, 0.2])):
        o = inp.pivoted_cholesky(x, 20, cov, 0.4, 1.3, lin=lin, ft=inp.LD)
        for mm in (1, 7, 20):
            want = inp.nystrom_trace(x, o['pivots'][:mm], cov, 0.4, 1.3, lin)
            assert abs(float(o['trace'][mm] - want)) <= 1e-13 * float(o['trace'][0])


def test_oracle_floor_ties_and_forced_pivots():
    base = _problem(10, 2, 4)
    x = np.repeat(base, 3, axis=0)
    o = inp.pivoted_cholesky(x, 14, inp.COV_MATERN12, 0.5, 1.3, floor=1e-9)
    assert o['rank'] == 10 and len(set(o['pivots'].tolist())) == 14
    assert not o['lt'][10:].any() and np.isfinite(o['lt']).all()
    forced = inp.pivoted_cholesky(x, 5, inp.COV_MATERN12, 0.5, 1.3, pivots=[4, 9, 20, 1, 13])
    assert forced['pivots'].tolist() == [4, 9, 20, 1, 13]
    assert forced['gaps'].shape == (5,) and (forced['best'] >= forced['at']).all()
    d = np.array([1.0, np.nan, 3.0, 3.0, 2.0])
    assert inp.pick(d, np.zeros(5, dtype=bool))[0] == 2
    assert inp.pick(d, np.array([0, 0, 1, 1, 0], dtype=bool))[0] == 4
    assert inp.pick(np.array([np.nan, np.nan]), np.array([1, 0], dtype=bool))[0] == 1


def test_clustered_fixture_shows_the_gap_in_numpy():
    """The issue's table: on clustered 1-D data greedy rows beat stride and random rows by a difference of kind."""
    n, m, ell, noise = 3000, 40, 0.15, 0.01
    x = inp.clustered(n, 0)
    y = np.sin(3 * x) + 0.1 * np.random.default_rng(1).normal(size=(n, 1))
    greedy = inp.pivoted_cholesky(x, m, inp.COV_RBF, ell, 1.0)
    bound, slack = inp.vfe_bound(x, y, greedy['pivots'], inp.COV_RBF, ell, 1.0, noise)
    assert abs(slack - float(greedy['trace'][m])) <= 1e-3 * n          # the jitter's share of the slack
    others = [((2 * np.arange(m) + 1) * n) // (2 * m)] + [np.random.RandomState(s).permutation(n)[:m] for s in range(10)]
    for rows in others:
        b, s = inp.vfe_bound(x, y, rows, inp.COV_RBF, ell, 1.0, noise)
        assert bound > b and slack < s
