"""Wrappers of include/cimrgp_psi.h, cimrgp_psi_grad.h and cimrgp_psi_rows.h: the psi statistics of the RBF covariance under
Gaussian inputs ("Sparse GP regression on uncertain inputs").  Each is one ``device._call``, as the wrappers of
``device.py`` are."""
import torch

from .device import _byte_scratch, _call, _given, _size, alloc_matrix


def _operands(mu, s, z, ell):
    """(n, m, d) of the operands, which must be contiguous and of one dtype; ``ell``: device float64 (d,)."""
    if mu.dim() != 2 or s.shape != mu.shape or z.dim() != 2 or z.shape[1] != mu.shape[1]:
        raise ValueError("mu and s must be (n, d) and z (m, d)")
    if s.dtype != mu.dtype or z.dtype != mu.dtype:
        raise ValueError("mu, s and z must have one dtype")
    if not (mu.is_contiguous() and s.is_contiguous() and z.is_contiguous()):
        raise ValueError("mu, s and z must be contiguous")
    if ell.dtype != torch.float64 or ell.numel() != mu.shape[1] or not ell.is_contiguous() or ell.device != mu.device:
        raise ValueError("ell must hold the d length-scales as float64 on the operands' device")
    return int(mu.shape[0]), int(z.shape[0]), int(mu.shape[1])


def psi1(mu, s, z, ell, sf2, out=None):
    """Psi1 (n x m) = E k(x, Z) for x_i ~ N(mu_i, diag s_i) into ``out`` or a new padded buffer (cimrgp_psi1)."""
    n, m, d = _operands(mu, s, z, ell)
    if out is None:
        out = alloc_matrix(n, m, mu.dtype, mu.device)
    _call("cimrgp_psi1", mu.dtype, mu, s, z, n, m, d, ell, sf2, out, out.stride(0))
    return out


def psi2_slices(n, m):
    """The number of row slices cimrgp_psi2 cuts n rows into for m inducing inputs (the header's rule); 0 outside its limits."""
    return _size("cimrgp_psi2_slices", n, m)


def psi2_scratch_bytes(n, m, d, dtype):
    return _size("cimrgp_psi2_scratch_bytes", dtype, n, m, d)


def psi2(mu, s, z, ell, sf2, out=None, scratch=None, bad=None):
    """lower(out)[:m, :m] = Psi2 = sum_i E k(Z, x_i) k(x_i, Z) (cimrgp_psi2).  Returns (out, bad): out is allocated with a
    padded pitch if None, the scratch for this call only if None; bad: device float64 (1,), the number of rows with a
    negative or non-finite variance (they add nothing)."""
    n, m, d = _operands(mu, s, z, ell)
    if out is None:
        out = alloc_matrix(m, m, mu.dtype, mu.device)
    bad = _given(bad, (1,), mu, torch.float64)
    scratch = _byte_scratch(psi2_scratch_bytes(n, m, d, mu.dtype), mu.device, scratch)
    _call("cimrgp_psi2", mu.dtype, mu, s, z, n, m, d, ell, sf2, out, out.stride(0), scratch, scratch.numel(), bad)
    return out, bad


def _weights(g, rows, cols, like):
    """``g``: the weight matrix of a gradient call, at least (rows, cols), of ``like``'s dtype, unit column stride."""
    if g.dim() != 2 or g.shape[0] < rows or g.shape[1] < cols or g.dtype != like.dtype or g.device != like.device or g.stride(1) != 1:
        raise ValueError("the weight matrix must be a (%d x %d) row-major matrix of the operands' dtype on their device" % (rows, cols))


def psi1_grad_scratch_bytes(n, m, d, dtype):
    return _size("cimrgp_psi1_grad_scratch_bytes", dtype, n, m, d)


def psi1_grad(mu, s, z, ell, sf2, g1, dmu=None, ds=None, dz=None, sums=None, scratch=None):
    """The derivatives of sum g1 o Psi1 for the weights g1 (n x m, any pitch) (cimrgp_psi1_grad, include/cimrgp_psi_grad.h).
    Returns (dmu (n, d), ds (n, d), dz (m, d), sums): sums device float64[d + 1] = [d/dlog sf2, d/dlog l_e ..]; every output
    is overwritten and allocated if None, the scratch for this call only if None."""
    n, m, d = _operands(mu, s, z, ell)
    _weights(g1, n, m, mu)
    dmu, ds, dz = _given(dmu, (n, d), mu), _given(ds, (n, d), mu), _given(dz, (m, d), mu)
    sums = _given(sums, (d + 1,), mu, torch.float64)
    scratch = _byte_scratch(psi1_grad_scratch_bytes(n, m, d, mu.dtype), mu.device, scratch)
    _call("cimrgp_psi1_grad", mu.dtype, mu, s, z, n, m, d, ell, sf2, g1, g1.stride(0), dmu, ds, dz, sums, scratch, scratch.numel())
    return dmu, ds, dz, sums


def psi2_grad_scratch_bytes(n, m, d, dtype):
    return _size("cimrgp_psi2_grad_scratch_bytes", dtype, n, m, d)


def psi2_grad(mu, s, z, ell, sf2, g2, dmu=None, ds=None, dz=None, sums=None, scratch=None, bad=None):
    """The derivatives of sum g2 o Psi2 for the SYMMETRIC weights g2 (m x m, any pitch; only its lower triangle is read)
    (cimrgp_psi2_grad).  Returns (dmu, ds, dz, sums, bad) as :func:`psi1_grad` and :func:`psi2` have them: sums[0] =
    2 sum g2 o Psi2; a row with a negative or non-finite variance is counted in bad and has zeros in dmu and ds."""
    n, m, d = _operands(mu, s, z, ell)
    _weights(g2, m, m, mu)
    dmu, ds, dz = _given(dmu, (n, d), mu), _given(ds, (n, d), mu), _given(dz, (m, d), mu)
    sums = _given(sums, (d + 1,), mu, torch.float64)
    bad = _given(bad, (1,), mu, torch.float64)
    scratch = _byte_scratch(psi2_grad_scratch_bytes(n, m, d, mu.dtype), mu.device, scratch)
    _call("cimrgp_psi2_grad", mu.dtype, mu, s, z, n, m, d, ell, sf2, g2, g2.stride(0), dmu, ds, dz, sums, scratch, scratch.numel(), bad)
    return dmu, ds, dz, sums, bad


def psi2_rows_quad_scratch_bytes(n, m, d, q, dtype):
    return _size("cimrgp_psi2_rows_quad_scratch_bytes", dtype, n, m, d, q)


def psi2_rows_quad(mu, s, z, ell, sf2, c, a, tr=None, quad=None, scratch=None, bad=None):
    """Per row i its own Psi2_i = E k(Z, x_i) k(x_i, Z), contracted and never stored (cimrgp_psi2_rows_quad,
    include/cimrgp_psi_rows.h): tr[i] = sum c o Psi2_i for the SYMMETRIC weights c (m x m, any pitch; only its lower triangle
    is read) and quad[i][k] = a_k^T Psi2_i a_k for the columns of a (m x q, any pitch).  Returns (tr (n,), quad (n, q), bad):
    every output is overwritten and allocated if None, the scratch for this call only if None; a row with a negative or
    non-finite variance is counted in bad (device float64 (1,)) and has zeros in tr and quad.  A row's results do not
    depend on n or on where the row lies in the operands."""
    n, m, d = _operands(mu, s, z, ell)
    _weights(c, m, m, mu)
    if a.dim() != 2 or a.shape[0] < m:
        raise ValueError("a must be an (m x q) matrix")
    q = int(a.shape[1])
    _weights(a, m, q, mu)
    tr, quad = _given(tr, (n,), mu), _given(quad, (n, q), mu)
    if quad.dim() != 2 or quad.stride(1) != 1 or tr.dim() != 1 or tr.stride(0) != 1:
        raise ValueError("tr must be a contiguous (n,) vector and quad a row-major (n x q) matrix")
    bad = _given(bad, (1,), mu, torch.float64)
    scratch = _byte_scratch(psi2_rows_quad_scratch_bytes(n, m, d, q, mu.dtype), mu.device, scratch)
    _call("cimrgp_psi2_rows_quad", mu.dtype, mu, s, z, n, m, d, ell, sf2, c, c.stride(0), a, a.stride(0), q, tr, quad, quad.stride(0),
          scratch, scratch.numel(), bad)
    return tr, quad, bad
