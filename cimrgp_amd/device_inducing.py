"""Wrappers of include/cimrgp_inducing.h: greedy inducing-point selection, the matrix-free pivoted Cholesky factorisation of
K(X, X) stopped after m columns ("Greedy inducing-point selection").  One ``device._call`` per wrapper, as the
wrappers of ``device.py`` are; FP64 only."""
import torch

from . import _lib
from .device import _byte_scratch, _call, _cov_id, _given, _size, padded_ld
from .device_linear import _lin_ok


def pivoted_cholesky_scratch_bytes(n, m):
    return _size("cimrgp_pivoted_cholesky_scratch_bytes", n, m)


def pivoted_cholesky(x, m, ell, sf2, lin=None, floor=0.0, cov=_lib.COV_RBF, pivots=None, lt=None, diag=None, trace=None, rank=None,
                     scratch=None):
    """The first ``m`` steps of the pivoted Cholesky factorisation of K(x, x), k = k_cov(ell, sf2) (+ sum_e lin[e] x_e x'_e
    with ``lin``, a device float64 (d,) tensor): ``(pivots (m,) int64, lt (m x ld) float64 whose row j is column j of L,
    diag (n,), trace (m + 1,), rank (1,) int64)``, all on the device and nothing read back (cimrgp_pivoted_cholesky).  An
    output that is not given is allocated, ``lt`` with a padded pitch; the scratch for this call only if None."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    n, d = x.shape
    if x.dtype != torch.float64:
        raise ValueError("pivoted_cholesky is built for float64 inputs only")
    if not 1 <= int(m) <= int(n):
        raise ValueError("m must be in [1, n], got m = %d for n = %d" % (int(m), int(n)))
    if lin is not None:
        _lin_ok(lin, d)
    pivots = _given(pivots, (m,), x, torch.int64)
    if lt is None:
        lt = torch.empty((int(m), padded_ld(n)), dtype=x.dtype, device=x.device)
    diag = _given(diag, (n,), x)
    trace = _given(trace, (int(m) + 1,), x)
    rank = _given(rank, (1,), x, torch.int64)
    scratch = _byte_scratch(pivoted_cholesky_scratch_bytes(n, m), x.device, scratch)
    _call("cimrgp_pivoted_cholesky", x.dtype, cov, x, n, d, ell, sf2, lin, m, floor, pivots, lt, lt.stride(0), diag, trace, rank,
          scratch, scratch.numel())
    return pivots, lt, diag, trace, rank
