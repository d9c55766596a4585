"""The memory footprint of include/cimrgp_sparse_ard.h (Guarded / run_contract of tests/test_gpu_buffer_contract.py), in the
manner of tests/test_gpu_sparse_grad_contract.py: padding columns of G and the rows below it poisoned, xa and xb end where a
guard begins, guards around every output and the scratch, const inputs keep their bytes; only sums[0 .. d] and db[nb x d]
change, and either output alone is the same bits."""
import numpy as np
import pytest

import sparse_ard_numpy as sa
from test_gpu_buffer_contract import (CONST, CUDA, INOUT, JUNK, OUT, TDT, Guarded, _call, _const_vec, _dt, _host, _lib, _out_vec,
                                      _round, _stream, _sync, dev, run_contract, wide_ld)  # noqa: F401
from test_gpu_sparse_contract import UNIT, _a_buf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("na,nb,d,cov", [(1, 1, 1, 0), (37, 16, 2, 1), (600, 130, 3, 2), (2049, 257, 8, 3), (130, 130, 2, 0)])
def test_cov_pair_grad_ard_footprint(dev, dt, acc, na, nb, d, cov):
    """Columns >= nb and rows >= na of G and rows >= na of xa are never read (NaN in one run), xa, xb and G keep their
    bytes, the scratch is written before it is read; with accumulate the outputs start from preset values."""
    tdt = TDT[dt]
    rng = np.random.default_rng(na + nb + d)
    xa = _round(rng.uniform(-2, 2, size=(na, d)) / np.sqrt(d), tdt)
    xb = xa if na == nb else _round(rng.uniform(-2, 2, size=(nb, d)) / np.sqrt(d), tdt)
    g = _round(rng.normal(size=(na, nb)), tdt)
    pre_s, pre_db = _round(rng.normal(size=1 + d), torch.float64), _round(rng.normal(size=(nb, d)), tdt)
    xab, xbb = _const_vec("xa", xa, tdt), _const_vec("xb", xb, tdt)
    gb = _a_buf("G", g, tdt)
    sums = _out_vec("sums", 1 + d, torch.float64, pre=pre_s if acc else None)
    db = _out_vec("db", nb * d, tdt, pre=pre_db if acc else None)
    lib = _lib().load()
    nbytes = int(lib.cimrgp_cov_pair_grad_ard_scratch_bytes(na, nb, d))
    assert nbytes == sa.pair_scratch_bytes(na, nb, d)
    scratch = Guarded("scratch", nbytes // 8, torch.float64, CUDA).vec(JUNK, nbytes // 8)

    def call(sums_ptr, db_ptr):
        _call(lib.cimrgp_cov_pair_grad_ard(_dt(tdt), cov, xab.ptr(), na, xbb.ptr(), nb, d, gb.ptr(), gb.ld, 0.7, 1.3, -2.0, acc,
                                           sums_ptr, db_ptr, scratch.ptr(), nbytes, _stream()), "cimrgp_cov_pair_grad_ard")

    run_contract([xab, xbb, gb, sums, db, scratch], lambda: call(sums.ptr(), db.ptr()), _sync)
    (s_ref, db_ref), (s_mag, db_mag) = sa.pair_grad_ard(xa, xb, g, cov, 0.7, 1.3, scale=-2.0)
    # the factor of tests/test_gpu_sparse_grad_contract.py: (na + 2) u for the sums and 4 x 170 u for the covariance's own error
    factor = (na + 2 + 4 * 170) * UNIT[dt]
    if acc:
        s_ref, db_ref, s_mag, db_mag = s_ref + pre_s, db_ref + pre_db, s_mag + np.abs(pre_s), db_mag + np.abs(pre_db)
    assert (np.abs(_host(sums.data) - s_ref) <= factor * s_mag + 1e-300).all()
    assert (np.abs(_host(db.data).reshape(nb, d) - db_ref) <= factor * db_mag + 1e-300).all()
    # sums_dev or db_dev NULL: the other gets the same bits, and the one left out keeps its own (run_contract checks that
    # nothing but the outputs changes: the buffer left out is not an output of that call)
    both_s, both_db = sums.data.clone(), db.data.clone()
    for b in (xab, xbb, gb, sums, db, scratch):
        b.fill("nan", seed=5)
    _sync()
    kept = db.data.clone()
    call(sums.ptr(), None)
    _sync()
    assert torch.equal(sums.data.view(torch.int64), both_s.view(torch.int64))
    assert torch.equal(db.full.view(torch.uint8), db.before.view(torch.uint8)) and torch.equal(kept.view(torch.uint8),
                                                                                              db.data.view(torch.uint8))
    for b in (xab, xbb, gb, scratch):
        b.check_unchanged("nan")
    for b in (xab, xbb, gb, sums, db, scratch):
        b.fill("nan", seed=6)
    _sync()
    call(None, db.ptr())
    _sync()
    assert torch.equal(db.data.view(torch.uint8), both_db.view(torch.uint8))
    assert torch.equal(sums.full.view(torch.uint8), sums.before.view(torch.uint8))
    for b in (xab, xbb, gb, scratch):
        b.check_unchanged("nan")
