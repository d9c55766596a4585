"""Wrappers of include/cimrgp_svgp.h: the variational sparse GP's row pass and its two m-sized moments (DESIGN.md,
"Variational sparse GP with a Student-t likelihood").  Each is one ``device._call``, as the wrappers of ``device.py`` are."""
import torch

from . import _lib
from .device import _byte_scratch, _call, _given, _same_pitch, _size, alloc_matrix


def svgp_rows_scratch_doubles(n):
    """Doubles of scratch cimrgp_svgp_rows needs for its sums: 3 (n + ceil(n / CIMRGP_SVGP_SUM_CHUNK))."""
    return 3 * (int(n) + (int(n) + _lib.SVGP_SUM_CHUNK - 1) // _lib.SVGP_SUM_CHUNK)


def svgp_rows(abuf, wbuf, n, m, gamma, kdiag, y, nodes, likelihood, s2, nu=0.0, mean=None, var=None, g1=None, g2=None, sums=None,
              want=("mean", "var", "g1", "g2", "sums")):
    """The variational sparse GP's row pass for ONE output column (cimrgp_svgp_rows): from A = abuf[:n, :m], W =
    wbuf[:n, :m], gamma (m,), kdiag (n,) and the targets ``y`` -- a 1-d view of n elements, e.g. a column of an (n, q) array,
    read in place through its stride -- the latent moments ``mean`` and ``var``, g1 = dE / dm, g2 = dE / dv (n,) and sums =
    [sum E, sum dE / dlog s2, #(v <= 0)] (device float64[3]).  ``nodes``: device float64 (2 H,), the Gauss-Hermite nodes then
    their weights.  Returns the outputs named in ``want`` as a dict; one that is wanted and not given is allocated, and so
    is the scratch of the sums, for this call only."""
    _same_pitch(abuf, wbuf, "abuf and wbuf")
    if y.dim() != 1 or y.numel() < int(n) or y.dtype != abuf.dtype or y.stride(0) < 1:
        raise ValueError("y must be a 1-d view of n elements of the matrices' dtype")
    for t, count, what in ((gamma, m, "gamma must hold m elements"), (kdiag, n, "kdiag must hold n elements")):
        if t.dtype != abuf.dtype or t.numel() < int(count) or not t.is_contiguous():
            raise ValueError(what + " of the matrices' dtype")
    if nodes.dtype != torch.float64 or nodes.numel() % 2 or not nodes.is_contiguous():
        raise ValueError("nodes must hold the H nodes and the H weights as float64")
    given = dict(mean=mean, var=var, g1=g1, g2=g2)
    out = {k: _given(given[k], (n,), abuf) for k in given if k in want}
    scratch = None
    if "sums" in want:
        out["sums"] = _given(sums, (3,), abuf, torch.float64)
        scratch = torch.empty(svgp_rows_scratch_doubles(n), dtype=torch.float64, device=abuf.device)
    _call("cimrgp_svgp_rows", abuf.dtype, abuf, wbuf, n, m, abuf.stride(0), gamma, kdiag, y, y.stride(0), nodes, nodes.numel() // 2,
          likelihood, s2, nu, out.get("mean"), out.get("var"), out.get("g1"), out.get("g2"), out.get("sums"), scratch)
    return out


def svgp_moments_scratch_bytes(n, m, q, dtype):
    return _size("cimrgp_svgp_moments_scratch_bytes", dtype, n, m, q)


def svgp_moments(abuf, n, m, w, r=None, out=None, g=None, scratch=None):
    """lower(out)[:m, :m] = A^T diag(w) A and, with ``r`` (n x q), g (m x q) = A^T r -- r NOT weighted -- from one pass
    over A = abuf[:n, :m] (cimrgp_svgp_moments).  Returns (out, g), allocated as :func:`device.wsyrk_tn` allocates them."""
    dtype = abuf.dtype
    q = 0 if r is None else int(r.shape[1])
    if out is None:
        out = alloc_matrix(m, m, dtype, abuf.device)
    if r is not None:
        g = _given(g, (m, q), abuf)
    scratch = _byte_scratch(svgp_moments_scratch_bytes(n, m, q, dtype), abuf.device, scratch)
    _call("cimrgp_svgp_moments", dtype, abuf, n, m, abuf.stride(0), w, r, q, out, out.stride(0), g, scratch, scratch.numel())
    return out, g
