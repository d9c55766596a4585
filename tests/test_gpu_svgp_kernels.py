"""GPU tests of include/cimrgp_svgp.h at the level of the two entry points, both dtypes and both likelihoods.
cimrgp_svgp_rows against an extended-precision NumPy evaluation (tests/svgp_numpy.quadrature, row_moments) under the
roundings-count rule of tests/test_gpu_sparse_post.py, its invariance to n and to the row's place, its count of bad rows;
cimrgp_svgp_moments against cimrgp_wsyrk_tn bit for bit and its a = A^T r at the componentwise bound; and the memory
footprint of both (Guarded / run_contract of tests/test_gpu_buffer_contract.py)."""
import numpy as np
import pytest

import svgp_numpy as so
from cimrgp_amd import device_svgp as devs
from test_gpu_buffer_contract import (CONST, CUDA, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec, _round,
                                      _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401
from test_gpu_sparse_contract import _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
U64 = 2.0 ** -53
#: (n, m): one row; four row tiles, m not a multiple of 64; three column tiles of the moments; many columns per lane
SHAPES = [(1, 16), (255, 100), (600, 257), (257, 1000)]
#: more than one chunk of the sums over the rows (2048 rows each), the last one ragged
SUM_SHAPE = (4500, 70)
LIKS = {"gaussian": 0, "student_t": 1}
S2, NU, H = 0.05, 3.0, 20
#: roundings the quadrature sums may be off their extended-precision value, in units of u times the sum of the magnitudes of
#: a sum's terms: 10 x the 6.6 that FP64 NumPy spends on the same four sums against numpy.longdouble over these shapes, both
#: dtypes' inputs and both likelihoods (measured once, on the host: E 6.5, g1 6.4, g2 6.6, gs 5.7)
Q_ROUNDINGS = 66.0


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", TDT[dt]).contiguous()


def rows_problem(n, m, dt, seed):
    """A, W (n x m), gamma (m), kdiag (n), y (n): the values the device holds, as float64 arrays.  sum A^2 ~ 0.5, sum W^2 ~
    0.3 against kdiag ~ 1.3: v stays well above 0.  Every seventh target is an outlier, far in the Student-t's tail."""
    rng = np.random.default_rng(seed)
    tdt = TDT[dt]
    a = _round(rng.normal(size=(n, m)) * np.sqrt(0.5 / m), tdt)
    w = _round(rng.normal(size=(n, m)) * np.sqrt(0.3 / m), tdt)
    gamma = _round(rng.normal(size=m), tdt)
    kdiag = _round(1.3 + 0.2 * rng.uniform(size=n), tdt)
    y = rng.normal(size=n)
    y[::7] += 4.0
    return a, w, gamma, kdiag, _round(y, tdt)


def _padded(a, dt, dev):
    buf = dev.alloc_matrix(a.shape[0], a.shape[1], TDT[dt], "cuda")
    buf.fill_(float("nan"))
    buf[:a.shape[0], :a.shape[1]] = _dev(a, dt)
    return buf


def _nodes():
    from cimrgp_amd.SVGP import hermite_nodes
    return torch.as_tensor(hermite_nodes(H)).to("cuda")


def _run_rows(dev, dt, lik, a, w, gamma, kdiag, y, **kw):
    n, m = a.shape
    out = devs.svgp_rows(_padded(a, dt, dev), _padded(w, dt, dev), n, m, _dev(gamma, dt), _dev(kdiag, dt), _dev(y, dt), _nodes(),
                        LIKS[lik], S2, NU, **kw)
    torch.cuda.synchronize()
    return out


def rows_bounds(a, w, gamma, kdiag, y, lik, dt):
    """The extended-precision values of the seven row quantities and the bound on the device's error in each:
    the row sums' (m + 2) u sum |terms|, carried to first order into the quadrature sums (the reference re-evaluated at
    m +- dm and v +- dv), plus Q_ROUNDINGS u sum |terms| of the quadrature itself, plus the rounding of the stored value."""
    m = a.shape[1]
    ld = np.longdouble
    mean, var, mmag, vmag = so.row_moments(a, w, gamma, kdiag, ld)
    dm, dv = (m + 2) * U64 * mmag, (m + 2) * U64 * vmag
    ref, mag = so.quadrature(lik, y, mean, var, S2, NU, ld, H)
    shifted = [so.quadrature(lik, y, mean + sm * dm, var + sv * dv, S2, NU, ld, H)[0] for sm, sv in ((1, 0), (-1, 0), (0, 1), (0, -1))]
    bounds = {}
    for k in ref:
        carried = sum(np.maximum(np.abs(shifted[i][k] - ref[k]), np.abs(shifted[i + 1][k] - ref[k])) for i in (0, 2))
        bounds[k] = carried + Q_ROUNDINGS * U64 * mag[k] + UNIT[dt] * np.abs(ref[k])
    ref["mean"], ref["var"] = mean, var
    bounds["mean"], bounds["var"] = dm + UNIT[dt] * np.abs(mean), dv + UNIT[dt] * np.abs(var)
    return ({k: np.asarray(v, dtype=np.float64) for k, v in ref.items()}, {k: np.asarray(v, dtype=np.float64) for k, v in bounds.items()},
            {k: np.asarray(v, dtype=np.float64) for k, v in mag.items()})


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lik", sorted(LIKS))
@pytest.mark.parametrize("n,m", SHAPES + [SUM_SHAPE])
def test_svgp_rows_within_the_roundings_of_its_sums(dev, dt, lik, n, m):
    a, w, gamma, kdiag, y = rows_problem(n, m, dt, n + m)
    ref, bound, mag = rows_bounds(a, w, gamma, kdiag, y, lik, dt)
    assert ref["var"].min() > 0.3
    out = _run_rows(dev, dt, lik, a, w, gamma, kdiag, y)
    worst = {}
    for k in ("mean", "var", "g1", "g2"):
        got = out[k].double().cpu().numpy()
        assert np.isfinite(got).all()
        worst[k] = float((np.abs(got - ref[k]) / bound[k]).max())
    sums = out["sums"].cpu().numpy()
    # the sums over the rows: FP64, never rounded to the dtype; (n + 2) u sum |terms| for adding them up
    for j, k in ((0, "E"), (1, "gs")):
        b = (bound[k] - UNIT[dt] * np.abs(ref[k])).sum() + (n + 2) * U64 * np.abs(ref[k]).sum()
        worst["sum " + k] = float(abs(sums[j] - ref[k].sum()) / b)
    print("svgp_rows %s %s (%d, %d): err/bound %s" % (dt, lik, n, m, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert sums[2] == 0.0 and max(worst.values()) <= 1.0
    if lik == "student_t" and n > 1:                      # not log-concave: g2 takes both signs
        assert bool((out["g2"] > 0).any()) and bool((out["g2"] < 0).any())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lik", sorted(LIKS))
def test_a_rows_results_do_not_depend_on_n_or_its_place_and_repeat(dev, dt, lik):
    n, m = 600, 257
    a, w, gamma, kdiag, y = rows_problem(n, m, dt, 11)
    whole = _run_rows(dev, dt, lik, a, w, gamma, kdiag, y)
    again = _run_rows(dev, dt, lik, a, w, gamma, kdiag, y)
    for k in whole:
        assert torch.equal(_bits(whole[k]), _bits(again[k])), k
    for i in (0, 3, 257, 599):                             # alone (n = 1, row 0 of its own launch)
        alone = _run_rows(dev, dt, lik, a[i:i + 1], w[i:i + 1], gamma, kdiag[i:i + 1], y[i:i + 1])
        for k in ("mean", "var", "g1", "g2"):
            assert torch.equal(_bits(alone[k]), _bits(whole[k][i:i + 1])), (k, i)
    part = _run_rows(dev, dt, lik, a[130:471], w[130:471], gamma, kdiag[130:471], y[130:471])          # another place, another n
    for k in ("mean", "var", "g1", "g2"):
        assert torch.equal(_bits(part[k]), _bits(whole[k][130:471])), k
    # y read in place through its stride: column 1 of an (n, 3) array
    y3 = torch.full((n, 3), float("nan"), dtype=TDT[dt], device="cuda")
    y3[:, 1] = _dev(y, dt)
    strided = devs.svgp_rows(_padded(a, dt, dev), _padded(w, dt, dev), n, m, _dev(gamma, dt), _dev(kdiag, dt), y3[:, 1], _nodes(),
                            LIKS[lik], S2, NU)
    for k in whole:
        assert torch.equal(_bits(strided[k]), _bits(whole[k])), k
    # outputs that are not wanted are not needed by the others
    few = _run_rows(dev, dt, lik, a, w, gamma, kdiag, y, want=("g2", "sums"))
    assert sorted(few) == ["g2", "sums"] and torch.equal(_bits(few["g2"]), _bits(whole["g2"]))
    assert torch.equal(_bits(few["sums"]), _bits(whole["sums"]))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lik", sorted(LIKS))
def test_rows_with_a_variance_that_is_not_positive_are_counted_and_add_nothing(dev, dt, lik):
    """kdiag lowered below sum A^2 - sum W^2 on three rows (one of them to NaN): arithmetic only, nothing faults."""
    n, m = 255, 100
    a, w, gamma, kdiag, y = rows_problem(n, m, dt, 21)
    rows = [0, 100, 254]
    good = _run_rows(dev, dt, lik, a, w, gamma, kdiag, y)
    kd = kdiag.copy()
    kd[rows[0]], kd[rows[1]], kd[rows[2]] = -0.5, -2.0, np.nan
    out = _run_rows(dev, dt, lik, a, w, gamma, kd, y)
    sums = out["sums"].cpu().numpy()
    assert sums[2] == 3.0
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    for k in ("mean", "var", "g1", "g2"):
        assert torch.equal(_bits(out[k][keep]), _bits(good[k][keep])), k
    assert torch.equal(_bits(out["mean"]), _bits(good["mean"]))
    assert bool((out["g1"][rows] == 0).all()) and bool((out["g2"][rows] == 0).all())
    assert float(out["var"][rows[0]]) < 0 and float(out["var"][rows[1]]) < 0 and bool(torch.isnan(out["var"][rows[2]]))
    # the other two sums are those of the remaining rows alone
    rest = _run_rows(dev, dt, lik, a[keep], w[keep], gamma, kdiag[keep], y[keep])["sums"].cpu().numpy()
    ref, _, _ = rows_bounds(a[keep], w[keep], gamma, kdiag[keep], y[keep], lik, dt)
    for j, k in ((0, "E"), (1, "gs")):
        assert np.isfinite(sums[j]) and abs(sums[j] - rest[j]) <= (n + 2) * U64 * np.abs(ref[k]).sum()


def _signed_weights(n, tdt, seed):
    """Weights of mixed sign with exact zeros, as the Student-t's g2 has them."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=n)
    w[::5] = 0.0
    return _round(w, tdt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m", SHAPES + [(5000, 130)])
def test_svgp_moments_is_wsyrk_tn_bit_for_bit_with_an_unweighted_a(dev, dt, n, m):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + 3 * m)
    a = _round(rng.normal(size=(n, m)), tdt)
    w, r = _signed_weights(n, tdt, n), _round(rng.normal(size=(n, 2)), tdt)
    ab, wd, rd = _padded(a, dt, dev), _dev(w, dt), _dev(r, dt)
    nmat, avec = devs.svgp_moments(ab, n, m, wd, rd)
    nmat2, avec2 = devs.svgp_moments(ab, n, m, wd, rd)
    twin, gtwin = dev.wsyrk_tn(ab, n, m, wd, rd)
    bare, none = devs.svgp_moments(ab, n, m, wd)
    bare_twin, _ = dev.wsyrk_tn(ab, n, m, wd)
    torch.cuda.synchronize()
    tri = torch.tril(torch.ones(m, m, dtype=torch.bool, device="cuda"))
    assert none is None
    for other in (nmat2, twin, bare, bare_twin):
        assert torch.equal(_bits(nmat[:m, :m][tri]), _bits(other[:m, :m][tri]))
    assert torch.equal(_bits(avec), _bits(avec2))
    assert devs.svgp_moments_scratch_bytes(n, m, 2, tdt) == dev.wsyrk_tn_scratch_bytes(n, m, 2, tdt)
    ld = np.longdouble
    ref = np.asarray(a, dtype=ld).T @ np.asarray(r, dtype=ld)
    mag = np.abs(np.asarray(a, dtype=ld)).T @ np.abs(np.asarray(r, dtype=ld))
    got = avec.double().cpu().numpy()
    worst = float((np.abs(got - ref) / ((n + 2) * UNIT[dt] * mag)).max())
    # the weighted g of the twin is another quantity
    assert n == 1 or not torch.equal(_bits(avec), _bits(gtwin))
    nref = (np.asarray(a, dtype=ld) * np.asarray(w, dtype=ld)[:, None]).T @ np.asarray(a, dtype=ld)
    nmag = (np.abs(np.asarray(a, dtype=ld)) * np.abs(np.asarray(w, dtype=ld))[:, None]).T @ np.abs(np.asarray(a, dtype=ld))
    il = np.tril_indices(m)
    worst_n = float((np.abs(nmat[:m, :m].double().cpu().numpy() - nref)[il] / ((n + 2) * UNIT[dt] * nmag[il] + 1e-300)).max())
    print("svgp_moments %s (%d, %d): a err/bound %.3f, N err/bound %.3f" % (dt, n, m, worst, worst_n))
    assert worst <= 1.0 and worst_n <= 1.0


# ---- the memory footprint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lik", sorted(LIKS))
@pytest.mark.parametrize("n,m", SHAPES + [SUM_SHAPE])
def test_svgp_rows_footprint(dev, dt, lik, n, m):
    """Padding columns and the rows below A and W are poisoned, y is one column of an (n, 3) array whose other columns are
    poisoned, the vectors end where a guard begins, the outputs sit between guards and the scratch is the call's own."""
    tdt, q, col = TDT[dt], 3, 1
    a, w, gamma, kdiag, y = rows_problem(n, m, dt, n + m + 1)
    ab, wb = _a_buf("A", a, tdt), _a_buf("W", w, tdt)
    gb, kb = _const_vec("gamma", gamma, tdt), _const_vec("kdiag", kdiag, tdt)
    mask = torch.zeros((n, q), dtype=torch.bool)
    mask[:, col] = True
    yb = Guarded("y", n * q, tdt, CUDA, ld=q).mark(CONST, n, q, part=mask, values=np.repeat(y[:, None], q, axis=1))
    from cimrgp_amd.SVGP import hermite_nodes
    nb = _const_vec("nodes", hermite_nodes(H), torch.float64)
    outs = [_out_vec(name, n, tdt) for name in ("mean", "var", "g1", "g2")]
    sums = _out_vec("sums", 3, torch.float64)
    nscratch = devs.svgp_rows_scratch_doubles(n)
    assert nscratch == 3 * (n + (n + 2047) // 2048)
    scratch = Guarded("scratch", nscratch, torch.float64, CUDA).vec(JUNK, nscratch)
    lib = _lib().load()
    run_contract([ab, wb, gb, kb, yb, nb, sums, scratch] + outs,
                 lambda: _call(lib.cimrgp_svgp_rows(_dt(tdt), ab.ptr(), wb.ptr(), n, m, ab.ld, gb.ptr(), kb.ptr(), yb.ptr(col), q, nb.ptr(),
                                                    H, LIKS[lik], S2, NU, outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(),
                                                    sums.ptr(), scratch.ptr(), _stream()), "cimrgp_svgp_rows"), _sync)
    ref, bound, _ = rows_bounds(a, w, gamma, kdiag, y, lik, dt)
    for buf, k in zip(outs, ("mean", "var", "g1", "g2")):
        assert (np.abs(_host(buf.data) - ref[k]) <= bound[k]).all(), k
    assert _host(sums.data)[2] == 0.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,q", [(1, 16, 1), (255, 100, 1), (600, 257, 2), (257, 1000, 1)])
def test_svgp_moments_footprint(dev, dt, n, m, q):
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m + q)
    a = _round(rng.normal(size=(n, m)), tdt)
    w, r = _signed_weights(n, tdt, m), _round(rng.normal(size=(n, q)), tdt)
    c0 = _round(rng.normal(size=(m, m)), tdt)
    ab, wb, rb = _a_buf("A", a, tdt), _const_vec("w", w, tdt), _const_vec("r", r, tdt)
    ldc = wide_ld(m)
    cb = Guarded("C", (m + 3) * ldc, tdt, CUDA, ld=ldc).mark(CONST, m, m, part="upper", values=c0).mark(OUT, m, m, part="lower")
    gb = _out_vec("g", m * q, tdt)
    lib = _lib().load()
    nbytes = int(lib.cimrgp_svgp_moments_scratch_bytes(_dt(tdt), n, m, q))
    scratch = Guarded("scratch", nbytes // ab.esz, tdt, CUDA).vec(JUNK, nbytes // ab.esz)
    run_contract([ab, wb, rb, cb, scratch, gb],
                 lambda: _call(lib.cimrgp_svgp_moments(_dt(tdt), ab.ptr(), n, m, ab.ld, wb.ptr(), rb.ptr(), q, cb.ptr(), ldc, gb.ptr(),
                                                       scratch.ptr(), nbytes, _stream()), "cimrgp_svgp_moments"), _sync)
    got = _host(gb.data).reshape(m, q)
    assert (np.abs(got - a.T @ r) <= (n + 2) * UNIT[dt] * (np.abs(a).T @ np.abs(r))).all()
    assert np.array_equal(_host(cb.mat(m, m))[np.triu_indices(m, 1)], c0[np.triu_indices(m, 1)])
