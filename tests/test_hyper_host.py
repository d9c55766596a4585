"""The shared host rules of hyper-parameter learning (cimrgp_amd/Hyper.py) and ``with_values`` of the kernel classes:
CPU only, no device and no library call."""
import numpy as np
import pytest
import torch
from scipy.optimize import minimize

from cimrgp_amd import Hyper, device as dev
from cimrgp_amd.KernelClass import RBFKernel, DenseMaternKernel, SparseKernel

CENTRE = np.array([0.3, -1.2, 2.0])
WEIGHTS = np.array([1.0, 4.0, 0.25])


def quadratic(theta):
    """A concave 'lml' with its gradient."""
    return -float(np.sum(WEIGHTS * (theta - CENTRE) ** 2)), -2.0 * WEIGHTS * (theta - CENTRE)


# ---- minimize_lml -------------------------------------------------------------------------------------------------------------
def test_minimize_lml_is_scipys_own_run_on_the_negated_function():
    got = Hyper.minimize_lml(quadratic, np.zeros(3), 50)
    want = minimize(lambda t: tuple(-v for v in quadratic(t)), np.zeros(3), jac=True, method='L-BFGS-B', options=dict(maxiter=50))
    assert np.array_equal(got.x, want.x) and got.nfev == want.nfev and got.nit == want.nit and got.fun == want.fun
    assert np.allclose(got.x, CENTRE, atol=1e-6)
    assert Hyper.minimize_lml(quadratic, np.zeros(3), 2).nit == 2          # max_iters is SciPy's maxiter


def _failing_second_call(fail):
    seen = []

    def objective(theta):
        seen.append(theta.copy())
        if len(seen) == 2:
            return fail()
        return quadratic(theta)
    return seen, objective


def _raise_not_pd():
    raise np.linalg.LinAlgError('Matrix is not positive definite')


@pytest.mark.parametrize("fail", [_raise_not_pd, lambda: None], ids=["LinAlgError", "None"])
def test_minimize_lml_failed_point_scores_1e100_and_zero_gradient(fail):
    seen, objective = _failing_second_call(fail)
    got = Hyper.minimize_lml(objective, np.zeros(3), 50)
    # what SciPy was given: the same run with the score written out
    calls = []

    def spelled_out(theta):
        calls.append(theta.copy())
        if len(calls) == 2:
            return 1e100, np.zeros(3)
        lml, grad = quadratic(theta)
        return -lml, -grad
    want = minimize(spelled_out, np.zeros(3), jac=True, method='L-BFGS-B', options=dict(maxiter=50))
    assert len(seen) > 2                                                   # the run went on after the failed point
    assert len(seen) == len(calls) and all(np.array_equal(a, b) for a, b in zip(seen, calls))
    assert np.array_equal(got.x, want.x) and got.nfev == want.nfev and got.fun == want.fun


@pytest.mark.parametrize("fail", [_raise_not_pd, lambda: None], ids=["LinAlgError", "None"])
def test_minimize_lml_two_point_failure_score_is_the_scalar(fail):
    state = dict(calls=0)

    def objective(theta):
        state['calls'] += 1
        if state['calls'] == 6:                  # a point of the line search, after the first gradient's 1 + 3 evaluations
            return fail()
        return quadratic(theta)[0]

    count = dict(calls=0)

    def spelled_out(theta):
        count['calls'] += 1
        return 1e100 if count['calls'] == 6 else -quadratic(theta)[0]

    got = Hyper.minimize_lml(objective, np.zeros(3), 50, jac=None)
    want = minimize(spelled_out, np.zeros(3), jac=None, method='L-BFGS-B', options=dict(maxiter=50))
    assert state['calls'] == count['calls'] > 6
    assert np.array_equal(got.x, want.x) and got.nfev == want.nfev and got.fun == want.fun
    assert np.isscalar(got.fun) or np.ndim(got.fun) == 0


def test_minimize_lml_other_exceptions_propagate():
    def objective(theta):
        raise RuntimeError('cimrgp_potrf: schedule watchdog')
    with pytest.raises(RuntimeError, match='schedule watchdog'):
        Hyper.minimize_lml(objective, np.zeros(3), 5)


# ---- pack_theta / unpack_theta ------------------------------------------------------------------------------------------------
def test_theta_round_trip_isotropic():
    theta = Hyper.pack_theta(2.0, 0.5, 0.01)
    assert np.array_equal(theta, np.log([2.0, 0.5, 0.01]))
    ell, sf, noise = Hyper.unpack_theta(theta)
    assert isinstance(ell, float) and isinstance(sf, float) and isinstance(noise, float)
    assert (ell, sf, noise) == tuple(float(v) for v in np.exp(theta)[[1, 0, 2]])
    assert np.allclose([ell, sf, noise], [0.5, 2.0, 0.01], rtol=1e-15)


def test_theta_round_trip_ard_and_trailing_entries():
    ells = np.array([0.5, 1.0, 3.0])
    theta = Hyper.pack_theta(2.0, ells, 0.01)
    assert np.array_equal(theta, np.log([2.0, 0.5, 1.0, 3.0, 0.01]))
    z = np.array([-7.0, 0.0, 1e3, -0.25])                                 # Z entries: never exponentiated, never touched
    long = np.concatenate([theta, z])
    keep = long.copy()
    ell, sf, noise = Hyper.unpack_theta(long, 3)
    assert ell.shape == (3,) and np.array_equal(ell, np.exp(theta[1:4]))
    assert sf == float(np.exp(theta[0])) and noise == float(np.exp(theta[4]))
    assert np.array_equal(long, keep)
    ell[:] = -1.0                                                          # a fresh array: theta does not see it
    assert np.array_equal(long, keep)
    assert np.array_equal(Hyper.unpack_theta(long, 3)[0], np.exp(theta[1:4]))
    one = Hyper.unpack_theta(Hyper.pack_theta(2.0, [0.5], 0.01), 1)[0]     # ARD in one dimension is still an array
    assert one.shape == (1,)


# ---- unit_lengthscale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_unit_lengthscale(dtype):
    ls = np.array([0.3, 2.0, 7.0])
    x = torch.arange(15, dtype=dtype).reshape(3, 5).t()                    # (5 x 3), not contiguous
    assert not x.is_contiguous()
    scale, xs = Hyper.unit_lengthscale(x, ls)
    assert scale.dtype == dtype and torch.equal(scale, torch.tensor(1.0 / ls, dtype=torch.float64).to(dtype))
    assert xs.is_contiguous() and xs.dtype == dtype and torch.equal(xs, x * scale)
    assert torch.equal(Hyper.unit_lengthscale(x, list(ls))[1], xs)         # a sequence does as well as an array
    t = torch.ones((2, 3), dtype=dtype)
    ts = Hyper.scaled(t, scale)
    assert ts.is_contiguous() and torch.equal(ts, scale.expand(2, 3))


# ---- sum_block_objectives -------------------------------------------------------------------------------------------------------
def _blocks(raising):
    order = []

    def evaluate(l):
        order.append(l)
        if l in raising:
            raise raising[l]
        return 10.0 ** l, np.array([1.0, 2.0, 3.0]) * 10.0 ** l
    return order, evaluate


def test_sum_block_objectives_order_and_sums():
    order, evaluate = _blocks({})
    lml, grad, failure = Hyper.sum_block_objectives([2, 0, 1], evaluate)
    assert order == [2, 0, 1]
    assert lml == 111.0 and np.array_equal(grad, [111.0, 222.0, 333.0]) and failure == 0.0
    lml, grad, failure = Hyper.sum_block_objectives([], evaluate)
    assert lml == 0.0 and np.array_equal(grad, np.zeros(3)) and failure == 0.0


def test_sum_block_objectives_failures_are_skipped_and_the_largest_code_stays():
    not_pd = np.linalg.LinAlgError('Matrix is not positive definite')
    watchdog = RuntimeError('cimrgp_potrf: schedule watchdog (n = 512)')
    order, evaluate = _blocks({1: not_pd})
    lml, grad, failure = Hyper.sum_block_objectives(range(4), evaluate)
    assert order == [0, 1, 2, 3] and failure == 1.0
    assert lml == 1101.0 and np.array_equal(grad, [1101.0, 2202.0, 3303.0])
    for raising in ({0: watchdog, 2: not_pd}, {0: not_pd, 2: watchdog}):
        order, evaluate = _blocks(raising)
        lml, grad, failure = Hyper.sum_block_objectives(range(4), evaluate)
        assert order == [0, 1, 2, 3] and failure == float(dev.INFO_WATCHDOG) and dev.is_watchdog(failure)
        assert lml == 1010.0 and np.array_equal(grad, [1010.0, 2020.0, 3030.0])


def test_sum_block_objectives_other_runtime_errors_propagate():
    order, evaluate = _blocks({1: RuntimeError('hipErrorOutOfMemory')})
    with pytest.raises(RuntimeError, match='OutOfMemory'):
        Hyper.sum_block_objectives(range(3), evaluate)
    assert order == [0, 1]


# ---- with_values ------------------------------------------------------------------------------------------------------------------
def test_with_values_keeps_class_and_nu():
    k = RBFKernel(l=2.0, sf=3.0, noise=0.1).with_values(0.5, 1.5, None)
    assert type(k) is RBFKernel and (k.l, k.sf, k.noise, k.cov) == (0.5, 1.5, None, 0)
    for nu in (0.5, 1.5, 2.5):
        base = DenseMaternKernel(nu=nu, l=2.0, sf=3.0)
        k = base.with_values(0.5, 1.5, 0.01)
        assert type(k) is DenseMaternKernel and (k.nu, k.l, k.sf, k.noise, k.cov) == (nu, 0.5, 1.5, 0.01, base.cov)
        assert (base.l, base.sf, base.noise) == (2.0, 3.0, None)           # a new object: the old one is as it was
    s = SparseKernel(DenseMaternKernel(nu=2.5), num_inducing=7, approximation='vfe', jitter=1e-5, inducing='random', seed=4)
    t = s.with_values(0.5, 1.5, 0.01)
    assert type(t) is SparseKernel and type(t.kernel) is DenseMaternKernel and (t.nu, t.l, t.sf, t.noise) == (2.5, 0.5, 1.5, 0.01)
    assert (t.num_inducing, t.approximation, t.jitter, t.inducing, t.seed) == (7, 'vfe', 1e-5, 'random', 4)


@pytest.mark.parametrize("kernel", [RBFKernel(), DenseMaternKernel(nu=0.5)], ids=["rbf", "matern12"])
def test_with_values_refuses_what_the_constructors_refuse(kernel):
    with pytest.raises(ValueError, match='length-scale must be positive'):
        kernel.with_values(0.0, 1.0, None)
    with pytest.raises(ValueError, match='length-scale must be positive'):
        kernel.with_values(float('nan'), 1.0, None)
    with pytest.raises(ValueError, match='signal variance must be positive'):
        kernel.with_values(1.0, -1.0, 0.1)
