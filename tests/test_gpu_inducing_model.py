"""Greedy inducing-point selection above the kernel: the block-level quality on clustered data, ``select_inducing`` feeding
the plugins, and ``SparseKernel(inducing='greedy')`` as a layer of MultiResolutionGaussianProcess against the NumPy chain of
tests/sparse_layer_numpy.py run with the model's own rows ("Greedy inducing-point selection").

The stride and random twins of the model must give the bits they gave before the greedy rule existed:
tests/golden/inducing_twins.npz holds their predictions and training-point chains as recorded with the parent build (the
commit before 'greedy'), by the same code as :func:`_twin_outputs`."""
import os
import socket

import numpy as np
import pytest

import inducing_numpy as inp
import sparse_layer_numpy as sl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inducing_twins.npz")
N, NS, D, M = 701, 175, 2, 48
ELLS = (0.5, 0.25, 0.125)
ARD = np.array([1.0, 1.6])                 # the ARD variant: every layer's length-scales are ells[j] * ARD
NU = {2: 1.5}


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


# ---- quality ----------------------------------------------------------------------------------------------------------------
def test_greedy_rows_beat_stride_and_random_rows_on_clustered_data(ca):
    """n = 3000 clustered 1-D inputs, m = 40, RBF l = 0.15, sf = 1, noise 0.01, VFE: the bound with the greedy rows exceeds the
    bound with stride rows and with each random draw of seeds 0-9 -- an inequality, first in the NumPy restatement (the
    fixture itself shows the gap), then for ``SparseBlock`` with the device's own greedy rows."""
    from cimrgp_amd.Inducing import greedy_rows
    from cimrgp_amd.Sparse import SparseBlock
    n, m, ell, noise = 3000, 40, 0.15, 0.01
    x = inp.clustered(n, 0)
    y = np.sin(3 * x) + 0.1 * np.random.default_rng(1).normal(size=(n, 1))
    others = [((2 * np.arange(m) + 1) * n) // (2 * m)] + [np.random.RandomState(s).permutation(n)[:m] for s in range(10)]
    oracle = inp.pivoted_cholesky(x, m, inp.COV_RBF, ell, 1.0)
    want = inp.vfe_bound(x, y, oracle['pivots'], inp.COV_RBF, ell, 1.0, noise)[0]
    assert all(want > inp.vfe_bound(x, y, rows, inp.COV_RBF, ell, 1.0, noise)[0] for rows in others)

    device = ca.device.require_gpu()
    xd, yd = torch.as_tensor(x).to(device), torch.as_tensor(y).to(device)
    kernel = ca.RBFKernel(l=ell, sf=1.0, noise=noise)
    picked = greedy_rows(xd, m, kernel)

    def bound(rows):
        z = xd.index_select(0, rows if isinstance(rows, torch.Tensor) else torch.as_tensor(rows).to(device))
        return SparseBlock(xd, z, kernel, 'vfe').fit(yd).log_marginal_likelihood()

    got = bound(picked.rows)
    rest = [bound(rows) for rows in others]
    trace = picked.trace_numpy()
    print("VFE bound: greedy %.1f (NumPy %.1f), stride %.1f, best random %.1f; tr(K - Q) %.2f of %.0f"
          % (got, want, rest[0], max(rest[1:]), trace[m], trace[0]))
    assert all(got > b for b in rest)
    assert trace[m] < 0.01 * trace[0] and int(picked.rank.item()) == m


# ---- plugins ----------------------------------------------------------------------------------------------------------------
def test_select_inducing_feeds_the_plugins(ca):
    from cimrgp_amd.Inducing import select_inducing
    rng = np.random.default_rng(3)
    x = rng.normal(size=(400, 2)) * [2.0, 0.5] + [10.0, -3.0]
    y = np.sin(x[:, :1]) + 0.1 * rng.normal(size=(400, 1))
    z, rows, trace = select_inducing(x, 30, lengthscale=0.7)
    assert z.shape == (30, 2) and rows.shape == (30,) and trace.shape == (31,) and len(set(rows.tolist())) == 30
    assert np.array_equal(z, x[rows]) and (np.diff(trace) <= 0).all()
    xn = (x - x.mean(axis=0)) / x.std(axis=0)
    oracle = inp.pivoted_cholesky(xn, 30, inp.COV_RBF, 0.7, 1.0, ft=inp.LD)
    if inp.qualifies(oracle['gaps'], 1.0, True, 30, 400):
        assert rows.tolist() == oracle['pivots'].tolist()
    for cls in (ca.SGP_FITC, ca.SparseGP_RBF):
        gp = cls(num_inducing=30, lengthscale=0.7, Z=z)
        gp.fit([x, y])
        # Z goes through (Z - mean) / std and back: two roundings of numbers of the size of x
        assert np.abs(gp.inducing_inputs - x[rows]).max() <= 4 * inp.EPS * np.abs(x).max()
        assert np.isfinite(gp.predict(x[:5])).all()
    # tol: the shortest prefix that reaches it, and never more than num_inducing rows
    z2, rows2, trace2 = select_inducing(x, 30, lengthscale=0.7, tol=0.25)
    keep = int(np.nonzero(trace <= 0.25 * trace[0])[0][0])
    assert 1 <= keep < 30 and rows2.tolist() == rows[:keep].tolist() and trace2.tobytes() == trace[:keep + 1].tobytes()
    assert np.array_equal(z2, x[rows2])


def test_rows_for_a_tolerance_is_the_oracles(ca):
    from cimrgp_amd.Inducing import greedy_rows
    x = np.random.default_rng(1).uniform(size=(515, 3))                     # the RBF d = 3 case of the kernel tests
    oracle = inp.pivoted_cholesky(x, 64, inp.COV_RBF, 0.5, 1.3, ft=inp.LD)
    assert inp.qualifies(oracle['gaps'], 1.3, True, 64, 515)
    picked = greedy_rows(torch.as_tensor(x).to(ca.device.require_gpu()), 64, ca.RBFKernel(l=0.5, sf=1.3))
    rel = np.asarray(oracle['trace'] / oracle['trace'][0], dtype=np.float64)
    for tol in (0.5, 0.1, 0.02):
        want = int(np.nonzero(rel <= tol)[0][0])
        assert min(abs(rel[want] - tol), abs(rel[want - 1] - tol)) > 1e-9          # the fixture: no entry sits on the threshold
        assert picked.rows_for(tol) == want
    assert picked.rows_for(0.0) == 64 and picked.rows_for(1.0) == 0


# ---- the model --------------------------------------------------------------------------------------------------------------
#: 'rbf_vfe' is the root the feature was specified with (l = 0.5).  On these inputs its first steps are SATURATED ties even in
#: long double (a row five length-scales from every pivot keeps the residual sf exactly), so the oracle's gaps do not decide
#: its rows; 'rbf_wide_vfe' (l = 1.0) is the region chosen so that they do, and there the whole sequence is asserted.
VARIANTS = {
    'rbf_vfe': dict(cov=0, mode=1, ard=False, ells=ELLS),
    'rbf_wide_vfe': dict(cov=0, mode=1, ard=False, ells=(1.0, 0.5, 0.25)),
    'matern32_fitc': dict(cov=2, mode=0, ard=False, ells=ELLS),
    'ard_vfe': dict(cov=0, mode=1, ard=True, ells=ELLS),
}
DECIDED = ('rbf_wide_vfe',)
MODE = {0: 'fitc', 1: 'vfe'}
_MODELS = {}


def _kernels(ca, cov, mode, ard, ells=ELLS, inducing='greedy'):
    out = []
    for j, ell in enumerate(ells):
        l = ell * ARD if ard else ell
        base = ca.RBFKernel(l=l, sf=1.0) if cov == 0 else ca.DenseMaternKernel(nu=NU[cov], l=l, sf=1.0)
        out.append(ca.SparseKernel(base, num_inducing=M, approximation=MODE[mode], inducing=inducing, seed=3) if j == 0 else base)
    return out


def _model(ca, name, inducing='greedy', **kw):
    key = (name, inducing, tuple(sorted(kw.items())))
    if key not in _MODELS:
        x, y, _, _ = sl.problem(N, D, NS, 0)
        model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(N, sl.RES, sl.DIVIDER),
                                                  spectral_density_obj=_kernels(ca, inducing=inducing, **VARIANTS[name]), **kw)
        model.fit()
        _MODELS[key] = model
    return _MODELS[key]


def _numpy_inputs(name):
    """The inputs the NumPy chain runs on: normalised and, for the ARD variant, divided by ARD (every layer's length-scales
    are ells[j] * ARD, so that the isotropic chain at ells on x / ARD is the same model)."""
    x, y, xs, _ = sl.problem(N, D, NS, 0)
    xn, xsn = sl.normalise(x, xs)
    if VARIANTS[name]['ard']:
        xn, xsn = xn * (1.0 / ARD), xsn * (1.0 / ARD)
    return xn, y, xsn


def _chain(name, rows, form, monkeypatch):
    """sparse_layer_numpy.chain with ``rows`` as the root's inducing rows: ``inducing_rows`` is substituted for the call."""
    v = VARIANTS[name]
    xn, y, xsn = _numpy_inputs(name)
    e = v['ells']
    layers = [sl.Layer(v['cov'], e[0], 1.0, None, M, v['mode'], 1e-6, 'greedy'), sl.Layer(v['cov'], e[1]), sl.Layer(v['cov'], e[2])]
    with monkeypatch.context() as mp:
        mp.setattr(sl, 'inducing_rows', lambda layer, j, l, n: np.asarray(rows))
        return sl.chain(xn, y, sl.index_bounds(N), layers, xsn, sl.index_bounds(NS), include_noise=False, form=form)


@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_greedy_root_layer_matches_the_numpy_chain(ca, name, monkeypatch):
    v = VARIANTS[name]
    model = _model(ca, name)
    post = model.posterior_obj[0]
    assert type(post).__name__ == 'SparsePosterior' and [type(p).__name__ for p in model.posterior_obj[1:]] == ['DensePosterior'] * 2
    rows = post.inducing_rows(0)
    assert rows.dtype == np.int64 and rows.shape == (M,) and len(set(rows.tolist())) == M and 0 <= rows.min() and rows.max() < N
    # the rows are the NumPy greedy rows of the region's normalised inputs wherever the oracle's own gaps decide them
    xn, y, xsn = _numpy_inputs(name)
    oracle = inp.pivoted_cholesky(xn, M, v['cov'], v['ells'][0], 1.0, ft=inp.LD)
    decided = inp.qualifies(oracle['gaps'], 1.0, True, M, N)
    print("%s: the oracle's gaps decide the rows: %s (smallest %.3e)" % (name, decided, float(np.min(oracle['gaps'][1:]))))
    if name in DECIDED:
        assert decided
    if decided:
        assert rows.tolist() == oracle['pivots'].tolist()
    # ... and greedy up to rounding in any case (the kernel tests' delta)
    forced = inp.pivoted_cholesky(xn, M, v['cov'], v['ells'][0], 1.0, ft=inp.LD, pivots=rows, keep=True)
    f64 = inp.pivoted_cholesky(xn, M, v['cov'], v['ells'][0], 1.0, pivots=rows, keep=True)
    delta = max(100.0 * float(np.nanmax(np.abs(f64['ds'] - forced['ds']))), 8 * M * inp.EPS)
    assert float(np.max(forced['best'] - forced['at'])) <= delta
    # prediction and the chain at the training points, against the chain run with the model's own rows
    w = _chain(name, rows, 'woodbury', monkeypatch)
    tol = sl.tolerance(w, _chain(name, rows, 'dense', monkeypatch))
    xs = sl.problem(N, D, NS, 0)[2]
    idx = ca.IndexSetUniform(NS, sl.RES, sl.DIVIDER)
    mean, var = model.get_predicted_mean_and_var(xs, idx, include_noise=False)
    mean_n, var_n = model.get_predicted_mean_and_var(xs, idx)
    f_bar = model._f_bar_final.double().cpu().numpy()
    noise = np.zeros(NS)
    for blk, (a, b) in zip(w['blocks'][-1], sl.index_bounds(NS)[-1]):
        noise[a:b] = blk['noise']
    gaps = (float(np.abs(mean - w['mean']).max()), float(np.abs(var - w['var']).max()), float(np.abs(f_bar - w['f_bar']).max()),
            float(np.abs(var_n - (w['var'] + noise)).max()))
    print("%s: gap mean %.3e var %.3e f_bar %.3e var+noise %.3e   tolerance mean %.3e var %.3e f_bar %.3e" % ((name,) + gaps + tol))
    assert np.isfinite(mean).all() and (var > 0).all()
    assert gaps[0] <= tol[0] and gaps[1] <= tol[1] and gaps[2] <= tol[2] and gaps[3] <= tol[1]
    assert np.array_equal(mean_n, mean)


def _twin_outputs(ca, model):
    xs = sl.problem(N, D, NS, 0)[2]
    mean, var = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(NS, sl.RES, sl.DIVIDER))
    return dict(mean=mean, var=var, f_bar=model._f_bar_final.double().cpu().numpy(), rows=model.posterior_obj[0].inducing_rows(0))


@pytest.mark.parametrize('rule', ['stride', 'random'])
def test_stride_and_random_twins_keep_their_bits(ca, rule):
    gold = np.load(GOLDEN)
    got = _twin_outputs(ca, _model(ca, 'rbf_vfe', inducing=rule))
    for what, value in got.items():
        assert np.asarray(value).tobytes() == gold['%s_%s' % (rule, what)].tobytes(), (rule, what)


def _rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as td
    import cimrgp_amd as ca
    torch.cuda.set_device(0)
    td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    ca.dist.share_one_gpu()
    model = _model(ca, 'rbf_vfe')
    xs = sl.problem(N, D, NS, 0)[2]
    out = dict(owner0=np.asarray(model.owner[0]))
    out['mean'], out['var'] = model.get_predicted_mean_and_var(xs, ca.IndexSetUniform(NS, sl.RES, sl.DIVIDER))
    out['f_bar'] = model._f_bar_final.double().cpu().numpy()
    try:                                   # the rows live on the rank that owns the region; the other rank never selected any
        out['rows'] = model.posterior_obj[0].inducing_rows(0)
    except RuntimeError as e:
        assert 'no greedy rows yet' in str(e) and int(model.owner[0][0]) != rank
        out['rows'] = np.zeros(0, dtype=np.int64)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    td.barrier()
    td.destroy_process_group()


def test_two_ranks_give_the_one_rank_rows_and_prediction(ca, tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    one = _twin_outputs(ca, _model(ca, 'rbf_vfe'))
    for r in range(2):
        g = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        # the root has one region: its owner selected the rows, and they are the one-rank rows; the prediction is every rank's
        assert g['rows'].tolist() == (one['rows'].tolist() if int(g['owner0'][0]) == r else [])
        assert g['mean'].tobytes() == one['mean'].tobytes() and g['var'].tobytes() == one['var'].tobytes()
        # (the chain's last layers are exact: 1e-12, the bar of the other two-rank tests, as in test_gpu_sparse_layer.py)
        assert float(np.abs(g['f_bar'] - one['f_bar']).max() / np.abs(one['f_bar']).max()) <= 1e-12


def test_learning_leaves_the_greedy_rows_where_they_are(ca):
    before = _model(ca, 'rbf_vfe').posterior_obj[0].inducing_rows(0)
    x, y, _, _ = sl.problem(N, D, NS, 0)
    model = ca.MultiResolutionGaussianProcess([x, y], index_set_obj=ca.IndexSetUniform(N, sl.RES, sl.DIVIDER),
                                              spectral_density_obj=_kernels(ca, **VARIANTS['rbf_vfe']), optimize_hyperparameters=True,
                                              max_iters=3)
    with pytest.raises(RuntimeError, match='no greedy rows yet'):
        model.posterior_obj[0].inducing_rows(0)
    model.fit()
    k = model.posterior_obj[0].kernel
    assert k.inducing == 'greedy' and (k.l, k.sf) != (ELLS[0], 1.0)          # learned, and the rule kept
    assert model.posterior_obj[0].inducing_rows(0).tolist() == before.tolist()
    z = model.posterior_obj[0].blocks[0].z.double().cpu().numpy()
    assert np.array_equal(z, model.x[0][0].double().cpu().numpy()[before])
