"""Wrappers of include/cimrgp_sparse_linear.h: the sparse GP's calls with a linear term in the covariance,
k(x, x') = k_cov(x, x') + sum_e lin_e x_e x'_e ("A linear term for the sparse GP").  Each is one ``device._call``,
as the wrappers of ``device.py`` are; ``lin`` is always a device float64 (d,) tensor, for both dtypes."""
import torch

from . import _lib
from .device import _byte_scratch, _call, _cov_id, _given, _size, alloc_matrix


def _lin_ok(lin, d):
    if lin is None or lin.dtype != torch.float64 or lin.numel() != int(d) or not lin.is_contiguous():
        raise ValueError("lin must hold d float64 weights on the device")


def cov_gram_lin(x, ell, sf2, lin, diag_add=0.0, lower_only=False, out=None, cov=_lib.COV_RBF):
    """:func:`device.rbf_gram` with + sum_e lin[e] x_ie x_je in every element (cimrgp_cov_gram_lin)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    n, d = x.shape
    _lin_ok(lin, d)
    if out is None:
        out = alloc_matrix(n, n, x.dtype, x.device)
    _call("cimrgp_cov_gram_lin", x.dtype, cov, x, n, d, ell, sf2, lin, diag_add, out, out.stride(0), lower_only)
    return out


def cov_cross_lin(xa, xb, ell, sf2, lin, out=None, cov=_lib.COV_RBF):
    """:func:`device.rbf_cross` with + sum_e lin[e] xa_ie xb_je in every element (cimrgp_cov_cross_lin)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    nb = xb.shape[0]
    _lin_ok(lin, d)
    if out is None:
        out = alloc_matrix(na, nb, xa.dtype, xa.device)
    _call("cimrgp_cov_cross_lin", xa.dtype, cov, xa, na, xb, nb, d, ell, sf2, lin, out, out.stride(0))
    return out


def sparse_lambda_kd(abuf, n, m, kdiag, noise, mode, lam=None, w=None, sums=None):
    """:func:`device.sparse_lambda` with k(x_i, x_i) = kdiag[i] (n elements of abuf's dtype) in place of the constant sf2:
    sums = [sum log lam, sum (kdiag_i - q_i), #(lam <= 0)] (cimrgp_sparse_lambda_kd)."""
    if kdiag.dtype != abuf.dtype or kdiag.numel() < int(n) or not kdiag.is_contiguous():
        raise ValueError("kdiag must hold n elements of the matrix's dtype")
    lam, w = _given(lam, (n,), abuf), _given(w, (n,), abuf)
    sums = _given(sums, (3,), abuf, torch.float64)
    _call("cimrgp_sparse_lambda_kd", abuf.dtype, abuf, n, m, abuf.stride(0), kdiag, noise, mode, lam, w, sums)
    return lam, w, sums


def cov_pair_grad_lin_scratch_bytes(na, nb, d, ard):
    return _size("cimrgp_cov_pair_grad_lin_scratch_bytes", na, nb, d, ard)


def cov_pair_grad_lin(xa, xb, gbuf, ell, sf2, lin, ard=False, scale=1.0, accumulate=False, sums=None, lsums=None, db=None,
                      want_sums=True, want_lsums=True, want_db=True, cov=_lib.COV_RBF, scratch=None):
    """:func:`device.cov_pair_grad` (``ard`` false: sums float64[2]) or :func:`device.cov_pair_grad_ard` (float64[1 + d]) under
    k = k_cov + linear: sums hold the covariance part only, lsums (device float64[d]) (+)= sum_ij G_ij xa_ie xb_je, and db
    (+)= scale (the twin's sum + lin[e] (G^T xa)_je) (cimrgp_cov_pair_grad_lin).  Returns (sums, lsums, db); an output that is
    wanted and not given is allocated, the scratch for this call only if None."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    nb = xb.shape[0]
    _lin_ok(lin, d)
    if want_sums:
        sums = _given(sums, (1 + d if ard else 2,), xa, torch.float64, zeros=True)
    if want_lsums:
        lsums = _given(lsums, (d,), xa, torch.float64, zeros=True)
    if want_db:
        db = _given(db, (nb, d), xa, zeros=True)
    scratch = _byte_scratch(cov_pair_grad_lin_scratch_bytes(na, nb, d, ard), xa.device, scratch)
    _call("cimrgp_cov_pair_grad_lin", xa.dtype, cov, xa, na, xb, nb, d, gbuf, gbuf.stride(0), ell, sf2, ard, lin, scale, accumulate,
          sums if want_sums else None, lsums if want_lsums else None, db if want_db else None, scratch, scratch.numel())
    return sums, lsums, db
