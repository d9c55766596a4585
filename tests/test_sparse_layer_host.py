"""CPU tests of the sparse layers of the multiresolution model: the SparseKernel wrapper, the two rules for the inducing
rows, the two NumPy forms of the chain (tests/sparse_layer_numpy.py) against each other, and the chain with Z = X against
the all-exact chain."""
import numpy as np
import pytest

import sparse_layer_numpy as sl
from cimrgp_amd import DenseMaternKernel, MaternKernel, RBFKernel, SparseKernel


def test_sparse_kernel_forwards_the_base_kernel():
    k = SparseKernel(DenseMaternKernel(nu=1.5, l=0.5, sf=2.0, noise=0.1), num_inducing=7, approximation='VFE', jitter=1e-5,
                     inducing='random', seed=4)
    assert (k.l, k.sf, k.noise, k.cov, k.nu) == (0.5, 2.0, 0.1, 2, 1.5)
    assert (k.num_inducing, k.approximation, k.jitter, k.inducing, k.seed) == (7, 'vfe', 1e-5, 'random', 4)
    r = SparseKernel(RBFKernel(l=0.25))
    assert (r.l, r.sf, r.noise, r.cov) == (0.25, 1.0, None, 0)
    assert (r.num_inducing, r.approximation, r.jitter, r.inducing, r.seed) == (1000, 'fitc', 1e-6, 'stride', 0)
    assert not hasattr(r, 'nu')
    w = k.with_noise(0.3)
    assert isinstance(w, SparseKernel) and w is not k and isinstance(w.kernel, DenseMaternKernel)
    assert (w.noise, w.l, w.sf, w.nu, k.noise) == (0.3, 0.5, 2.0, 1.5, 0.1)
    assert (w.num_inducing, w.approximation, w.jitter, w.inducing, w.seed) == (7, 'vfe', 1e-5, 'random', 4)


def test_sparse_kernel_refuses_bad_arguments():
    base = RBFKernel()
    for bad in (MaternKernel(), SparseKernel(base), None, 1.0):
        with pytest.raises(TypeError):
            SparseKernel(bad)
    for kw in (dict(num_inducing=0), dict(num_inducing=-3), dict(approximation='svgp'), dict(jitter=-1e-9),
               dict(jitter=float('nan')), dict(inducing='kmeans')):
        with pytest.raises(ValueError):
            SparseKernel(base, **kw)
    for ok in ('fitc', 'vfe', 'dtc'):
        assert SparseKernel(base, approximation=ok, jitter=0.0, num_inducing=1).approximation == ok


#: (n, m) -> the rows floor((k + 0.5) n / m)
STRIDE = {
    (10, 4): [1, 3, 6, 8],
    (10, 1): [5],
    (7, 7): [0, 1, 2, 3, 4, 5, 6],
    (3, 5): [0, 1, 2],
    (1, 1000): [0],
    (11, 3): [1, 5, 9],
    (700, 130): None,
}


@pytest.mark.parametrize("n,m", sorted(STRIDE))
def test_stride_rule(n, m):
    rows = SparseKernel(RBFKernel(), num_inducing=m).inducing_rows(2, 1, n)
    assert rows.dtype == np.int64 and len(rows) == min(n, m)
    want = STRIDE[(n, m)]
    if want is not None:
        assert rows.tolist() == want
    mm = min(n, m)
    assert rows.tolist() == [int(np.floor((k + 0.5) * n / mm)) for k in range(mm)] == sl.stride_rows(n, mm).tolist()
    assert (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    # a function of n alone among (layer, region, seed)
    assert np.array_equal(rows, SparseKernel(RBFKernel(), num_inducing=m, seed=9).inducing_rows(0, 5, n))


def test_random_rule_depends_on_seed_layer_region_and_n_alone():
    k = SparseKernel(RBFKernel(), num_inducing=50, inducing='random', seed=3)
    rows = k.inducing_rows(1, 2, 400)
    assert np.array_equal(rows, np.random.RandomState([3, 1, 2]).permutation(400)[:50])
    assert len(set(rows.tolist())) == 50 and rows.dtype == np.int64
    # another object with the same settings, another base kernel, another approximation: the same rows
    other = SparseKernel(DenseMaternKernel(nu=0.5, l=3.0), num_inducing=50, inducing='random', seed=3, approximation='vfe')
    assert np.array_equal(rows, other.inducing_rows(1, 2, 400))
    assert np.array_equal(rows, k.with_noise(0.2).inducing_rows(1, 2, 400))
    # ... and each of seed, layer, region and n changes them
    for alt in (SparseKernel(RBFKernel(), 50, inducing='random', seed=4).inducing_rows(1, 2, 400), k.inducing_rows(0, 2, 400),
                k.inducing_rows(1, 3, 400), k.inducing_rows(1, 2, 401)):
        assert not np.array_equal(rows, alt)
    assert sorted(k.inducing_rows(0, 0, 20).tolist()) == list(range(20))         # m >= n: every row
    lay = sl.Layer(0, 1.0, m=50, inducing='random', seed=3)
    assert np.array_equal(rows, sl.inducing_rows(lay, 1, 2, 400))


def test_the_shapes_of_the_checks_are_ragged():
    b = sl.index_bounds(sl.N)
    assert [[hi - lo for lo, hi in layer] for layer in b] == [[2801], [1400, 1401], [700, 700, 700, 701]]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("d", [1, 2])
def test_the_two_oracle_forms_agree(d, cov, mode):
    """Both forms are backward stable in K_uu + eps sf I: 1e-9 is what tests/test_sparse_host.py allows them per block."""
    w = sl.case_chain(d, cov, mode)
    g = sl.gap(w, sl.case_chain(d, cov, mode, form='dense'))
    print("d=%d cov=%d mode=%d: gap mean %.3e var %.3e f_bar %.3e" % ((d, cov, mode) + g))
    assert max(g) <= 1e-9
    assert np.isfinite(w['mean']).all() and (w['var'] > 0).all()


def test_the_two_oracle_forms_agree_with_all_layers_sparse_and_random_rows():
    kw = dict(sparse=(0, 1, 2), inducing='random')
    g = sl.gap(sl.case_chain(2, 0, 0, **kw), sl.case_chain(2, 0, 0, form='dense', **kw))
    print("all sparse, random: gap mean %.3e var %.3e f_bar %.3e" % g)
    assert max(g) <= 1e-9


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [1, 2])
def test_inducing_at_the_data_is_the_all_exact_chain(d, mode):
    """m >= n, eps = 0, Matern 1/2: Z = X in every block, Q_ff = K_ff, so the sparse chain is the exact one."""
    s = sl.case_chain(d, 1, mode, sparse=(0, 1), m=4000, eps=0.0)
    e = sl.case_chain(d, 1, mode, sparse=())
    assert s['blocks'][0][0]['rows'].tolist() == list(range(sl.N))
    g = sl.gap(s, e)
    print("Z = X d=%d mode=%d: gap mean %.3e var %.3e f_bar %.3e" % ((d, mode) + g))
    assert max(g) <= 1e-10
