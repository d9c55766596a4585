"""The expectations of test_gpu_potrf_failure.py, confirmed by LAPACK on the CPU: for every injected-pivot case of
potrf_failure_numpy (n <= 6144, injected value -1.0 or 0.0) dpotrf returns info == j exactly, and so does spotrf on
the float32 copy of the matrix -- the construction leaves no room for a rounding-level +-1."""
import numpy as np
import pytest
import scipy.linalg as sla

import oracle
import potrf_failure_numpy as pf

_GRAMS = {}


def _gram(n, seed):
    """The clean base matrix, computed once per (n, seed) (only the largest is worth keeping)."""
    key = (n, seed)
    if key not in _GRAMS:
        if n >= 2048:
            _GRAMS.clear()
        _GRAMS[key] = pf.base_gram(pf.points(n, seed))
    return _GRAMS[key]


def _case_id(case):
    n, seed, inj = case
    return "n%d-s%d-%s" % (n, seed, "+".join("j%d(%g)" % (j, v) for j, v in inj))


@pytest.mark.parametrize("case", pf.host_cases(), ids=_case_id)
def test_lapack_reports_the_injected_pivot_in_both_precisions(case):
    n, seed, inj = case
    k = _gram(n, seed)
    want = pf.expected_info(inj)
    kbad = pf.inject(k, inj)
    # leading minors of order < j are those of the clean matrix
    assert np.array_equal(kbad[:want - 1, :want - 1], k[:want - 1, :want - 1])
    _, info64 = sla.lapack.dpotrf(kbad, lower=1)
    assert info64 == want
    _, info32 = sla.lapack.spotrf(kbad.astype(np.float32), lower=1)
    assert info32 == want


def test_the_case_lists_cover_what_the_gpu_file_runs():
    """Every single-matrix and batched case with n <= 6144 and a value of -1.0 or 0.0 has its host check; the others
    (NaN, n = 10240) are the ones the helper leaves out on purpose."""
    host = pf.host_cases()
    assert len(host) == len(set(host))
    left_out = [(n, inj) for n, _, inj in pf.single_cases() if (n, n, inj) not in host]
    assert left_out == [(700, ((300, pf.NAN),)), (pf.PAIRED[0], ((pf.PAIRED[1], -1.0),))]
    for n, _, bad in pf.BATCHED:
        for blk, j in bad.items():
            assert (n, pf.batch_seed(n, blk), ((j, -1.0),)) in host
    # j = 1, 64, 65, 256, 257, 641 and 700 at n = 700: every block boundary of the one-queue cases is there
    assert {inj[0][0] for n, _, inj in host if n == 700 and len(inj) == 1} >= {1, 2, 64, 65, 193, 256, 257, 448, 641, 700}


def test_two_injected_pivots_report_the_first():
    k = _gram(700, 700)
    for j1, j2 in ((100, 500), (64, 65), (256, 257)):
        kbad = pf.inject(k, ((j2, -1.0), (j1, -1.0)))
        assert sla.lapack.dpotrf(kbad, lower=1)[1] == j1
        assert sla.lapack.spotrf(kbad.astype(np.float32), lower=1)[1] == j1
        assert pf.expected_info(((j2, -1.0), (j1, -1.0))) == j1


def test_clean_pivots_stay_far_above_rounding():
    """What makes the index exact: the smallest pivot of the clean matrix (the squared diagonal of its factor) is of the
    order of the noise, 0.1 -- six orders of magnitude above FP32 rounding of entries of size 1."""
    for n in (700, 3584):
        lmat, info = oracle.potrf_lower(_gram(n, n))
        assert info == 0
        assert float(np.min(np.diag(lmat)) ** 2) >= pf.NOISE


def test_column_ranges():
    assert [pf.block_start(j) for j in (1, 64, 65, 256, 257, 641, 700)] == [0, 0, 64, 192, 256, 640, 640]
    assert [pf.panel_start(j) for j in (1, 256, 257, 512, 513, 6144)] == [0, 0, 256, 256, 512, 5888]


def test_staged_duplicate_point_fails_at_the_duplicate():
    """The staged pipeline's bad block (the failure comes through the inputs): a duplicated point, ell about the spacing,
    no noise.  dpotrf reports exactly the duplicate's order; without the duplicate the matrix is well conditioned."""
    x = pf.staged_bad_points()
    j = pf.STAGED_J
    _, info = oracle.potrf_lower(oracle.rbf_gram(x, None, pf.STAGED_ELL, 1.1, 0.0))
    assert info == j
    xc = np.linspace(-2.0, 2.0, pf.STAGED_N).reshape(-1, 1)
    lmat, info = oracle.potrf_lower(oracle.rbf_gram(xc[:j + 64], None, pf.STAGED_ELL, 1.1, 0.0))
    assert info == 0
    assert float(np.min(np.diag(lmat)) ** 2) > 0.5
