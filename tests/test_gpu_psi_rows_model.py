"""GPU tests of the predictive variance at uncertain test inputs above the kernel ("Predictive variance at
uncertain test inputs"): ``UncertainInputBlock.predict_moments`` and ``BayesianGPLVM.predict_uncertain`` against the oracle
of tests/psi_rows_numpy.py, on the problem of tests/test_gpu_psi_model.py (NS test rows, their variances over three decades
with every fourth row exactly 0).

The rule is the project's standing one, as tests/test_gpu_psi_model.py states and applies it (its ``_within``; the same
figures as ``psi_numpy.allowance``): every case evaluates the oracle in float64 and in longdouble and allows a device
quantity 10 x |float64 - longdouble| of that quantity off the longdouble value, never less than 1e-10 relative; a vector or a
matrix (a prediction) is one quantity: both sides of the rule are its largest entry.  The variance is sf - sum C o Psi2* + ..,
a difference of numbers of order sf in which C carries K_uu^-1 at jitter 1e-6: that cancellation, not the kernel, sets the
error, and the float64 oracle shows its size (DESIGN.md has the measured figures, also under the entry-by-entry reading of
the rule, which the mean of ``predict(xs_var=)`` itself does not meet)."""
import numpy as np
import pytest

import psi_numpy as po
import psi_rows_numpy as pr
from test_gpu_psi_model import NOISE, NS, _block, _dev, _problem, _within

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(32, 1, 1, False), (32, 3, 2, True), (70, 2, 2, True)]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _bits(t):
    return t.contiguous().view(torch.int64)


def _allowed(v64, vld):
    """The rule's allowance for the quantity whose oracle values are ``v64`` and ``vld``."""
    own = float(np.abs(np.asarray(v64, dtype=np.longdouble) - vld).max())
    return max(10.0 * own, 1e-10 * float(np.abs(vld).max()))


def _agree(a, b, allowed, what):
    diff = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    print("%s: difference %.3e, allowed %.3e" % (what, diff, allowed))
    return diff <= allowed


def _outputs(q, ns=NS):
    return torch.empty((ns, q), dtype=torch.float64, device="cuda"), torch.empty((ns, q), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("m,d,q,ard", CASES)
def test_predict_moments_matches_the_oracle(ca, m, d, q, ard):
    mu, s, z, y, ell, xs, xs_var, m64, mld = _problem(m, d, q, ard)
    blk = _block(ca, mu, _dev(s), z, ell, ard).fit(_dev(y))
    mean, var = _outputs(q)
    got = blk.predict_moments(_dev(xs), _dev(xs_var), mean, var)
    assert got[0] is mean and got[1] is var
    # the mean is predict(xs_var=)'s, bit for bit
    pmean = torch.empty_like(mean)
    blk.predict(_dev(xs), pmean, None, xs_var=_dev(xs_var))
    assert torch.equal(_bits(mean), _bits(pmean))
    (a64, v64), (ald, vld) = pr.moments(m64, xs, xs_var), pr.moments(mld, xs, xs_var)
    assert tuple(var.shape) == (NS, q) and bool((var > 0).all())
    ok = _within(mean.cpu().numpy(), a64, ald, "mean (%d, %d, %d)" % (m, d, q))
    ok &= _within(var.cpu().numpy(), v64, vld, "variance (%d, %d, %d)" % (m, d, q))
    # on the rows with xs_var = 0 every column is SparseBlock.predict's variance
    zero = np.flatnonzero((xs_var == 0).all(axis=1))
    assert len(zero) == NS // 4
    exact = torch.empty(NS, dtype=torch.float64, device="cuda")
    blk.predict(_dev(xs), None, exact)
    for c in range(q):
        ok &= _agree(var[:, c].cpu().numpy()[zero], exact.cpu().numpy()[zero], _allowed(v64, vld),
                     "variance at xs_var = 0, column %d, against SparseBlock.predict" % c)
    # either output alone, and the noise
    only_var = torch.empty_like(var)
    assert blk.predict_moments(_dev(xs), _dev(xs_var), None, only_var)[1] is only_var and torch.equal(_bits(only_var), _bits(var))
    only_mean = torch.empty_like(mean)
    assert blk.predict_moments(_dev(xs), _dev(xs_var), only_mean, None)[1] is None and torch.equal(_bits(only_mean), _bits(mean))
    noisy = _outputs(q)
    blk.predict_moments(_dev(xs), _dev(xs_var), *noisy, include_noise=True)
    assert torch.equal(_bits(noisy[1]), _bits(var + blk.kernel.noise)) and blk.kernel.noise == NOISE
    assert ok


def test_chunking_and_a_shared_variance_change_no_bits(ca):
    """``budget_bytes=1`` (chunks of 256 rows) gives the bits of one chunk; a shared (d,) variance the bits of its (ns, d)
    broadcast, a scalar those of its broadcast too."""
    m, d, q, ard = 70, 2, 2, True
    mu, s, z, y, ell, xs, xs_var, _, _ = _problem(m, d, q, ard)
    blk = _block(ca, mu, _dev(s), z, ell, ard).fit(_dev(y))
    ns = 600                                                      # three chunks of 256 rows, the last one ragged
    rng = np.random.RandomState(17)
    big, big_var = rng.randn(ns, d), 10.0 ** rng.uniform(-3, 0, size=(ns, d))
    big_var[::4] = 0.0
    assert blk.chunk_rows(1) == 256 and blk.chunk_rows() >= ns
    one, many = _outputs(q, ns), _outputs(q, ns)
    blk.predict_moments(_dev(big), _dev(big_var), *one)
    blk.predict_moments(_dev(big), _dev(big_var), *many, budget_bytes=1)
    assert torch.equal(_bits(one[0]), _bits(many[0])) and torch.equal(_bits(one[1]), _bits(many[1]))
    for shared in (np.array([0.3, 0.02]), 0.05):
        rows, vec = _outputs(q, ns), _outputs(q, ns)
        blk.predict_moments(_dev(big), _dev(np.broadcast_to(shared, (ns, d)).copy()), *rows)
        blk.predict_moments(_dev(big), shared, *vec, budget_bytes=1)
        assert torch.equal(_bits(rows[0]), _bits(vec[0])) and torch.equal(_bits(rows[1]), _bits(vec[1]))


def test_a_negative_test_variance_raises(ca):
    mu, s, z, y, ell, xs, xs_var, _, _ = _problem(32, 1, 1, False)
    blk = _block(ca, mu, _dev(s), z, ell, False).fit(_dev(y))
    bad = xs_var.copy()
    bad[3, 0], bad[17, 0] = -1e-3, np.nan
    with pytest.raises(ValueError, match="2 of the test rows"):
        blk.predict_moments(_dev(xs), _dev(bad), *_outputs(1))
    with pytest.raises(TypeError, match="not yet supported"):
        blk.predict(_dev(xs), _outputs(1)[0], torch.empty(NS, dtype=torch.float64, device="cuda"), xs_var=_dev(xs_var))


def test_plugin_predict_uncertain(ca):
    """``BayesianGPLVM(num_inducing=24)``: the mean is ``predict(test_var=)``'s, the variance the oracle's in z-scored units, and
    at test_var = 0 it is ``predict_with_variance``'s in every column."""
    from cimrgp_amd.GPLVM import BayesianGPLVM
    n, d, q = 300, 2, 2
    rng = np.random.RandomState(21)
    x = rng.uniform(-2.0, 3.0, size=(n, d)) * np.array([1.0, 4.0])
    y = np.sin(x @ rng.randn(d, q)) + 0.1 * rng.randn(n, q) + 2.0
    xs = rng.uniform(-2.0, 3.0, size=(NS, d)) * np.array([1.0, 4.0])
    tv = 10.0 ** rng.uniform(-3, 0, size=(NS, d)) * np.array([1.0, 16.0])
    tv[::4] = 0.0
    g = BayesianGPLVM(num_inducing=24)
    assert g.fit([x, y]) is True
    xm, xsd, ym, ysd = x.mean(axis=0), x.std(axis=0), y.mean(axis=0), y.std(axis=0)
    xn, yn, xsn = (x - xm) / xsd, (y - ym) / ysd, (xs - xm) / xsd
    zn = xn[np.random.RandomState(0).permutation(n)[:24]]
    m64, mld = po.both(xn, xn.var() * 0.01, zn, yn, np.ones(d), 1.0, 1.0, eps=1e-6)
    back = lambda a: np.asarray(a, dtype=np.longdouble) * ysd + ym
    mean, var = g.predict_uncertain(xs, tv)
    assert mean.shape == var.shape == (NS, q)
    assert np.array_equal(mean, g.predict(xs, test_var=tv))
    (a64, v64), (ald, vld) = pr.moments(m64, xsn, tv / xsd ** 2), pr.moments(mld, xsn, tv / xsd ** 2)
    ok = _within(mean, back(a64), back(ald), "plugin mean") and _within(var, v64, vld, "plugin variance (z-scored units)")
    _, noisy = g.predict_uncertain(xs, tv, include_noise=True, budget_bytes=1)
    assert np.array_equal(noisy, var + g.kernel.noise)
    # a shared variance, in the caller's units: the same model within the rule (its mean takes the per-row kernel)
    shared = np.array([0.04, 0.5])
    (a64, v64), (ald, vld) = pr.moments(m64, xsn, shared / xsd ** 2), pr.moments(mld, xsn, shared / xsd ** 2)
    smean, svar = g.predict_uncertain(xs, shared)
    ok &= _within(smean, back(a64), back(ald), "plugin mean (shared)") and _within(svar, v64, vld, "plugin variance (shared)")
    # test_var = 0: predict_with_variance's variance in every column
    _, zvar = g.predict_uncertain(xs, 0.0)
    pmean, pvar = g.predict_with_variance(xs)
    (_, p64), (_, pld) = m64.predict(xsn), mld.predict(xsn)
    for c in range(q):
        ok &= _within(zvar[:, c], p64, pld, "plugin variance at test_var = 0, column %d" % c)
        ok &= _agree(zvar[:, c], pvar, _allowed(p64, pld), "plugin variance at test_var = 0 against predict_with_variance, column %d" % c)
    assert ok
    with pytest.raises(ValueError, match="test_var"):
        g.predict_uncertain(xs, np.full((NS - 1, d), 0.1))
    with pytest.raises(ValueError, match="test_var"):
        g.predict_uncertain(xs, -0.1)
    with pytest.raises(TypeError, match="not yet supported"):
        g.predict_with_variance(xs, test_var=tv)
