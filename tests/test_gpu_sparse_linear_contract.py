"""The memory footprint of include/cimrgp_sparse_linear.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py), in the
manner of tests/test_gpu_sparse_post_contract.py: padding columns and the rows below every matrix are poisoned (NaN in one run,
random values in the other), point arrays, the weights and the diagonal end where a guard begins, outputs and the scratch sit
between guards, const inputs keep their bytes, and the outputs are the same bits whatever the poison."""
import numpy as np
import pytest

import sparse_ard_numpy as sa
import sparse_linear_numpy as sl
from test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec,
                                      _round, _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401
from test_gpu_sparse_contract import UNIT, _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LIN = np.array([0.5, 0.2, 0.35, 0.11, 0.7, 0.05, 0.9, 0.41])
TOL = {"f64": 1e-13, "f32": 2e-6}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lower_only", [False, True])
@pytest.mark.parametrize("n,d", [(1, 1), (63, 2), (65, 3), (257, 8)])
def test_cov_gram_lin_footprint(dev, dt, n, d, lower_only):
    """As cimrgp_cov_gram's: the lower triangle (everything with lower_only = 0) is written and nothing right of column n or
    below row n; lower_only = 1 may write above the diagonal inside the n x n block.  lin is d doubles, no more."""
    tdt = TDT[dt]
    cov = (n + d) % 4
    rng = np.random.default_rng(n * 10 + d)
    x = _round(rng.uniform(-1.7, 1.7, size=(n, d)), tdt)
    xb, lb = _const_vec("x", x, tdt), _const_vec("lin", LIN[:d], torch.float64)
    kb = Guarded("K", (n + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n))
    kb.mark(OUT, n, n, part="lower").mark(JUNK if lower_only else OUT, n, n, part="upper")
    lib = _lib().load()
    run_contract([xb, lb, kb], lambda: _call(lib.cimrgp_cov_gram_lin(_dt(tdt), cov, xb.ptr(), n, d, 0.37, 1.9, lb.ptr(), 0.05, kb.ptr(),
                                                                     kb.ld, int(lower_only), _stream()), "cimrgp_cov_gram_lin"), _sync)
    ref = sl.ksum(x, x, cov, 0.37, 1.9, LIN[:d]) + 0.05 * np.eye(n)
    got = _host(kb.mat(n, n))
    if lower_only:
        got, ref = np.tril(got), np.tril(ref)
    assert np.max(np.abs(got - ref)) / np.abs(ref).max() < TOL[dt]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("na,nb,d", [(77, 201, 2), (1, 65, 3), (130, 1, 1), (257, 63, 8)])
def test_cov_cross_lin_footprint(dev, dt, na, nb, d):
    tdt = TDT[dt]
    cov = (na + d) % 4
    rng = np.random.default_rng(na + nb)
    xa = _round(rng.uniform(-1.5, 1.5, size=(na, d)), tdt)
    xbh = _round(rng.uniform(-1.5, 1.5, size=(nb, d)), tdt)
    ga, gb, lb = _const_vec("xa", xa, tdt), _const_vec("xb", xbh, tdt), _const_vec("lin", LIN[:d], torch.float64)
    kab = Guarded("Kab", (na + 3) * wide_ld(nb), tdt, CUDA, ld=wide_ld(nb)).mark(OUT, na, nb)
    lib = _lib().load()
    run_contract([ga, gb, lb, kab], lambda: _call(lib.cimrgp_cov_cross_lin(_dt(tdt), cov, ga.ptr(), na, gb.ptr(), nb, d, 0.8, 0.7, lb.ptr(),
                                                                           kab.ptr(), kab.ld, _stream()), "cimrgp_cov_cross_lin"), _sync)
    ref = sl.ksum(xa, xbh, cov, 0.8, 0.7, LIN[:d])
    assert np.max(np.abs(_host(kab.mat(na, nb)) - ref)) / np.abs(ref).max() < TOL[dt]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 1), (333, 70), (1030, 257)])
def test_sparse_lambda_kd_footprint(dev, dt, mode, n, m):
    """kdiag is n elements of the dtype, read whatever the mode (sums[1] needs it) and never written."""
    tdt = TDT[dt]
    rng = np.random.default_rng(n + m)
    a = _round(rng.normal(size=(n, m)) * 0.5 / np.sqrt(m), tdt)
    kd = _round(1.3 + rng.uniform(0.0, 2.0, size=n), tdt)
    ab, kb = _a_buf("A", a, tdt), _const_vec("kdiag", kd, tdt)
    lam, w = _out_vec("lam", n, tdt), _out_vec("w", n, tdt)
    sums = _out_vec("sums", 3, torch.float64)
    lib = _lib().load()
    run_contract([ab, kb, lam, w, sums], lambda: _call(lib.cimrgp_sparse_lambda_kd(_dt(tdt), ab.ptr(), n, m, ab.ld, kb.ptr(), 0.02, mode,
                                                                                   lam.ptr(), w.ptr(), sums.ptr(), _stream()),
                                                       "cimrgp_sparse_lambda_kd"), _sync)
    qd = (a * a).sum(axis=1)
    lam_ref = kd - qd + 0.02 if mode == 0 else np.full(n, 0.02)
    tol = 1e-14 if dt == "f64" else 1e-6
    assert np.abs(_host(lam.data) - lam_ref).max() <= tol * 4
    assert np.abs(_host(w.data) * _host(lam.data) - 1).max() <= 4 * UNIT[dt]
    s = _host(sums.data)
    assert s[2] == 0 and abs(s[0] - np.log(_host(lam.data)).sum()) <= 1e-13 * np.abs(np.log(_host(lam.data))).sum()
    assert abs(s[1] - (kd - qd).sum()) <= (1e-13 if dt == "f64" else 1e-6) * np.abs(kd - qd).sum()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ard", [0, 1])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("na,nb,d,cov", [(1, 1, 1, 0), (37, 16, 2, 1), (600, 130, 3, 2), (2049, 257, 8, 3), (130, 130, 2, 0)])
def test_cov_pair_grad_lin_footprint(dev, dt, ard, acc, na, nb, d, cov):
    """Columns >= nb and rows >= na of G and rows >= na of xa are never read, xa, xb, G and lin keep their bytes, the scratch
    (both partial arrays) is written before it is read; only sums, lsums[d] and db[nb x d] change; with accumulate they start
    from preset values; an output left out keeps its bytes and the others get the same bits."""
    tdt = TDT[dt]
    rng = np.random.default_rng(na + nb + d)
    xa = _round(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d), tdt)
    xb = xa if na == nb else _round(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d), tdt)
    g = _round(rng.normal(size=(na, nb)), tdt)
    ns = 1 + d if ard else 2
    pre_s, pre_l = _round(rng.normal(size=ns), torch.float64), _round(rng.normal(size=d), torch.float64)
    pre_db = _round(rng.normal(size=(nb, d)), tdt)
    xab, xbb, lb = _const_vec("xa", xa, tdt), _const_vec("xb", xb, tdt), _const_vec("lin", LIN[:d], torch.float64)
    gb = _a_buf("G", g, tdt)
    sums = _out_vec("sums", ns, torch.float64, pre=pre_s if acc else None)
    lsums = _out_vec("lsums", d, torch.float64, pre=pre_l if acc else None)
    db = _out_vec("db", nb * d, tdt, pre=pre_db if acc else None)
    lib = _lib().load()
    nbytes = int(lib.cimrgp_cov_pair_grad_lin_scratch_bytes(na, nb, d, ard))
    assert nbytes == sl.pair_scratch_bytes(na, nb, d, bool(ard))
    scratch = Guarded("scratch", nbytes // 8, torch.float64, CUDA).vec(JUNK, nbytes // 8)
    inputs, outputs = (xab, xbb, lb, gb, scratch), (sums, lsums, db)

    def call(sums_ptr, lsums_ptr, db_ptr):
        _call(lib.cimrgp_cov_pair_grad_lin(_dt(tdt), cov, xab.ptr(), na, xbb.ptr(), nb, d, gb.ptr(), gb.ld, 0.7, 1.3, ard, lb.ptr(), -2.0,
                                           acc, sums_ptr, lsums_ptr, db_ptr, scratch.ptr(), nbytes, _stream()), "cimrgp_cov_pair_grad_lin")

    run_contract(list(inputs + outputs), lambda: call(sums.ptr(), lsums.ptr(), db.ptr()), _sync)
    (s_ref, l_ref, db_ref, _), (s_mag, l_mag, dbl_mag) = sl.pair_grad_lin(xa, xb, g, cov, 0.7, 1.3, LIN[:d], bool(ard), scale=-2.0)
    # the factor of tests/test_gpu_sparse_grad_contract.py: (na + 2) u for the sums and 4 x 170 u for the covariance's own error
    factor = (na + 2 + 4 * 170) * UNIT[dt]
    (_, _), (_, dbc_mag) = sa.pair_grad_ard(xa, xb, g, cov, 0.7, 1.3, scale=-2.0)
    db_mag = dbc_mag + dbl_mag
    if acc:
        s_ref, l_ref, db_ref = s_ref + pre_s, l_ref + pre_l, db_ref + pre_db
        s_mag, l_mag, db_mag = s_mag + np.abs(pre_s), l_mag + np.abs(pre_l), db_mag + np.abs(pre_db)
    assert (np.abs(_host(sums.data) - s_ref) <= factor * s_mag + 1e-300).all()
    assert (np.abs(_host(lsums.data) - l_ref) <= (na + 2) * UNIT["f64"] * l_mag + 1e-300).all()
    assert (np.abs(_host(db.data).reshape(nb, d) - db_ref) <= factor * db_mag + 1e-300).all()
    # one output at a time: the same bits, and the ones left out keep theirs
    both = [o.data.clone() for o in outputs]
    for k, only in enumerate(outputs):
        for b in inputs + outputs:
            b.fill("nan", seed=5 + k)
        _sync()
        call(*[o.ptr() if o is only else None for o in outputs])
        _sync()
        assert torch.equal(only.data.view(torch.uint8), both[k].view(torch.uint8))
        for o in outputs:
            if o is not only:
                assert torch.equal(o.full.view(torch.uint8), o.before.view(torch.uint8))
        for b in (xab, xbb, lb, gb):
            b.check_unchanged("nan")
