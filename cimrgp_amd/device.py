"""Thin, typed wrappers around the C ABI operating on torch CUDA tensors.

torch is used for device memory, streams and (elsewhere) torch.distributed --
plumbing only; every arithmetic operation of the path below is a hand-written
HIP kernel reached through ``libcimrgp.so``.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def as_torch_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        if dtype not in _DT:
            raise ValueError("dtype must be float32 or float64")
        return dtype
    key = str(dtype).lower()
    if key in ("f64", "float64", "fp64", "double", "<class 'numpy.float64'>"):
        return torch.float64
    if key in ("f32", "float32", "fp32", "float", "<class 'numpy.float32'>"):
        return torch.float32
    raise ValueError("dtype must be 'f32' or 'f64', got %r" % (dtype,))


def require_gpu(device=None):
    """Resolve the device of the product path; there is no CPU fallback."""
    _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("cimrgp_amd: no HIP device visible; the dense GP path has no CPU fallback "
                           "(the NumPy restatement under oracle/ is test infrastructure only)")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def padded_ld(n):
    """Row pitch (elements): a multiple of 16 (every row starts on a 128-byte line) that is NOT a
    multiple of 512 elements: with a power-of-two pitch all rows of a tile start in the same HBM
    channel / cache set and the strided tile accesses of the update kernels serialise there."""
    ld = max(16, (int(n) + 15) // 16 * 16)
    if ld % 512 == 0:
        ld += 16
    return ld


def alloc_matrix(rows, cols, dtype, device):
    """(rows x cols) row-major view of a buffer with a padded leading dimension."""
    ld = padded_ld(cols)
    buf = torch.empty((max(int(rows), 1), ld), dtype=dtype, device=device)
    return buf


def to_device(a, dtype, device):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not isinstance(a, torch.Tensor) else a
    return t.to(device=device, dtype=dtype).contiguous()


def _cov_id(cov):
    cov = int(cov)
    if cov not in (_lib.COV_RBF, _lib.COV_MATERN12, _lib.COV_MATERN32, _lib.COV_MATERN52):
        raise ValueError("unknown covariance id %d (include/cimrgp.h CIMRGP_COV_*)" % cov)
    return cov


def rbf_gram(x, ell, sf2, diag_add=0.0, lower_only=False, out=None, cov=_lib.COV_RBF):
    """D1.  x: (n x d) device tensor.  Returns the (n x ld) buffer; [:, :n] is K.
    ``cov``: covariance id (``_lib.COV_*``, a kernel object's ``.cov``); every covariance, the RBF included, goes
    through cimrgp_cov_gram (bit-identical to cimrgp_rbf_gram for the RBF)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    n, d = x.shape
    if out is None:
        out = alloc_matrix(n, n, x.dtype, x.device)
    lib = _lib.load()
    _lib.check(lib.cimrgp_cov_gram(_DT[x.dtype], cov, _p(x), n, d, float(ell), float(sf2), float(diag_add),
                                   _p(out), out.stride(0), int(bool(lower_only)), _stream()), "cimrgp_cov_gram")
    return out


def rbf_cross(xa, xb, ell, sf2, out=None, cov=_lib.COV_RBF):
    """Cross-Gram (na x nb) into a padded buffer; ``cov`` as for :func:`rbf_gram`."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    nb = xb.shape[0]
    if out is None:
        out = alloc_matrix(na, nb, xa.dtype, xa.device)
    lib = _lib.load()
    _lib.check(lib.cimrgp_cov_cross(_DT[xa.dtype], cov, _p(xa), na, _p(xb), nb, d, float(ell), float(sf2),
                                    _p(out), out.stride(0), _stream()), "cimrgp_cov_cross")
    return out


def potrf_workspace_bytes(n, dtype):
    return int(_lib.load().cimrgp_potrf_workspace_bytes(_DT[dtype], int(n)))


def potrf_workspace(n, dtype, device):
    return torch.empty(max(potrf_workspace_bytes(n, dtype), 16), dtype=torch.uint8, device=device)


def potrf(kbuf, n, ws=None, info=None):
    """D2 in place on kbuf[:n, :n] (lower).  Returns (ws, info) -- info is a
    device int32 scalar written asynchronously (LAPACK convention)."""
    lib = _lib.load()
    if ws is None:
        ws = potrf_workspace(n, kbuf.dtype, kbuf.device)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=kbuf.device)
    _lib.check(lib.cimrgp_potrf(_DT[kbuf.dtype], _p(kbuf), int(n), kbuf.stride(0), _p(ws), ws.numel(),
                                _p(info), _stream()), "cimrgp_potrf")
    return ws, info


def potrf_rows(kbuf, n, bbuf, m, ws=None, info=None):
    """D2 with m carried rows: kbuf[:n,:n] = L L^T in place and bbuf[:m,:n] <- bbuf L^-T."""
    lib = _lib.load()
    if ws is None:
        ws = potrf_workspace(n, kbuf.dtype, kbuf.device)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=kbuf.device)
    _lib.check(lib.cimrgp_potrf_rows(_DT[kbuf.dtype], _p(kbuf), int(n), kbuf.stride(0), _p(ws), ws.numel(),
                                     _p(info), _p(bbuf), int(m), bbuf.stride(0), _stream()), "cimrgp_potrf_rows")
    return ws, info


def block_posterior(x, y, xs, ell, sf2, noise, kbuf, wbuf, ws, info, alpha, z, mean, var, add_noise=False, accumulate=False,
                    scratch=None, streams=None):
    """One block's whole posterior in ONE call (cimrgp_block_posterior, include/cimrgp.h): Gram matrix, factorisation with
    the cross-Gram rows and the targets carried, backward solve, predictive mean and variance -- the same kernels as the
    separate calls.  kbuf (n x ld), wbuf ((ns + q) x ld), ws / info as for potrf; alpha, z (n x q),
    mean (ns x q), var (ns) are filled.  ``scratch``: 2 q n elements (allocated here when not given: a caller that
    must not allocate between two events -- bench.py's timed step -- passes its own).
    ``streams`` = (front, factor, solve) torch streams: the three stages on three streams
    (cimrgp_block_posterior_staged), for callers that pipeline independent blocks over rotating buffer sets and order
    the reuse of a set themselves; results are then ordered on ``solve``."""
    lib = _lib.load()
    n, d = x.shape
    q = y.shape[1]
    ns = 0 if xs is None else xs.shape[0]
    if scratch is None:
        scratch = torch.empty(2 * q * max(int(n), 1), dtype=x.dtype, device=x.device)
    elif scratch.numel() < 2 * q * max(int(n), 1) or scratch.dtype != x.dtype:
        raise ValueError("scratch must hold 2 q n elements of the block's dtype")
    if streams is not None:
        sf, sp, sq = (s.cuda_stream for s in streams)
        _lib.check(lib.cimrgp_block_posterior_staged(_DT[x.dtype], _p(x), int(n), int(d), _p(y), int(q), _p(xs), int(ns), float(ell),
                                                     float(sf2), float(noise), _p(kbuf), kbuf.stride(0), _p(ws), ws.numel(), _p(info),
                                                     _p(wbuf), wbuf.stride(0), _p(alpha), _p(z), _p(scratch), _p(mean), _p(var),
                                                     int(bool(add_noise)), int(bool(accumulate)), sf, sp, sq),
                   "cimrgp_block_posterior_staged")
        return mean, var
    _lib.check(lib.cimrgp_block_posterior(_DT[x.dtype], _p(x), int(n), int(d), _p(y), int(q), _p(xs), int(ns), float(ell), float(sf2),
                                          float(noise), _p(kbuf), kbuf.stride(0), _p(ws), ws.numel(), _p(info), _p(wbuf),
                                          wbuf.stride(0), _p(alpha), _p(z), _p(scratch), _p(mean), _p(var), int(bool(add_noise)),
                                          int(bool(accumulate)), _stream()), "cimrgp_block_posterior")
    return mean, var


def _context_queue(entry, stream):
    """``entry`` (cimrgp_solve_queue / cimrgp_front_queue) for ``stream`` (default: the current stream), wrapped as a torch
    stream; ``stream`` itself when it owns no context."""
    cur = torch.cuda.current_stream() if stream is None else stream
    out = ctypes.c_void_p()
    _lib.check(getattr(_lib.load(), entry)(cur.cuda_stream, ctypes.byref(out)), entry)
    if (out.value or 0) == (cur.cuda_stream or 0):
        return cur
    return torch.cuda.ExternalStream(out.value, device=cur.device)


def solve_queue(stream=None):
    """The stream to pass as ``streams[2]`` of :func:`block_posterior` (cimrgp_solve_queue, include/cimrgp.h): the
    look-ahead context's queue that is idle between two factorisations on ``stream`` (default: the current stream),
    wrapped as a torch stream; ``stream`` itself when it owns no context."""
    return _context_queue("cimrgp_solve_queue", stream)


def front_queue(stream=None):
    """The stream to pass as ``streams[0]`` of :func:`block_posterior` when consecutive calls are independent blocks
    (cimrgp_front_queue, include/cimrgp.h): the look-ahead context's queue that falls idle before a factorisation on
    ``stream`` ends, wrapped as a torch stream; ``stream`` itself when it owns no context."""
    return _context_queue("cimrgp_front_queue", stream)


def potrf_rows_batched(karena, n, ld, ws_arena, info, barena=None, m=0, ldb=0):
    """``batch`` equal-sized factorisations in the same launches.  karena: (batch, n, ld) tensor,
    ws_arena: (batch, ws_bytes) uint8, info: (batch,) int32, barena: (batch, m, ldb) carried rows."""
    lib = _lib.load()
    batch = karena.shape[0]
    _lib.check(lib.cimrgp_potrf_rows_batched(_DT[karena.dtype], _p(karena), int(n), int(ld), karena.stride(0), _p(ws_arena),
                                             ws_arena.stride(0), _p(info), _p(barena), int(m), int(ldb),
                                             0 if barena is None else barena.stride(0), int(batch), _stream()),
               "cimrgp_potrf_rows_batched")


def solve_lt_batched(karena, n, ld, ws_arena, z):
    """Backward halves for a batch: z (batch, n, q) = L^-1 R is overwritten with alpha."""
    lib = _lib.load()
    batch, _, q = z.shape
    scratch = torch.empty((batch, 2 * q * max(int(n), 1)), dtype=karena.dtype, device=karena.device)
    _lib.check(lib.cimrgp_solve_lt_batched(_DT[karena.dtype], _p(karena), int(n), int(ld), karena.stride(0), _p(ws_arena),
                                           ws_arena.stride(0), _p(z), int(q), _p(scratch), int(batch), _stream()),
               "cimrgp_solve_lt_batched")
    return z


#: work areas of cimrgp_layer_fit (carried target rows, solve scratch) per (device, dtype, STREAM): the fit of a layer
#: is enqueue-only, so they are not allocated per call; a new shape replaces the cached one (O(batch q n) elements).
#: Keyed by the stream the call is enqueued on (round 5): two fits on two streams -- two models, two
#: threads, a caller's stream pool -- must not share the carried rows; within one stream the calls are ordered, and the
#: caching allocator frees a replaced area in that same stream's order.
_LAYER_WORK = {}


def _layer_work_areas(batch, q, n, ldr, dtype, device):
    key = (str(device), dtype, int(_stream() or 0))
    shape = (batch, q, n)
    hit = _LAYER_WORK.get(key)
    if hit is None or hit[0] != shape:
        rows = torch.empty((batch, q, ldr), dtype=dtype, device=device)
        scratch = torch.empty((batch, 2 * q * max(n, 1)), dtype=dtype, device=device)
        hit = (shape, rows, scratch)
        _LAYER_WORK[key] = hit
    return hit[1], hit[2]


def layer_fit(x, y, fbar, train_out, starts, n, ell, sf2, noise_fixed, noise_frac, noise_floor, shared_bias, shared_noise,
              karena, ws_arena, info, bias, noise, z, alpha, cov=_lib.COV_RBF):
    """The fit of ``batch`` equal-sized blocks of one layer in ONE call (cimrgp_layer_fit_cov, include/cimrgp.h).
    x, y, fbar, train_out: the LAYER's arrays (N x d / N x q); starts: device int64 (batch,) row offsets.
    karena (batch, n, ld), ws_arena (batch, ws_bytes) uint8, info (batch,) int32, bias (batch, q), noise (batch,),
    z / alpha (batch, n, q) are filled.  noise_fixed < 0: from the statistics (or ``shared_noise``)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(karena.shape[0])
    q = int(y.shape[1])
    d = int(x.shape[1])
    ldr = padded_ld(n)
    rows, scratch = _layer_work_areas(batch, q, int(n), ldr, y.dtype, y.device)
    _lib.check(lib.cimrgp_layer_fit_cov(_DT[y.dtype], cov, _p(x), _p(y), _p(fbar), _p(train_out), _p(starts), batch, int(n), d,
                                        q, float(ell), float(sf2), float(noise_fixed), float(noise_frac), float(noise_floor),
                                        _p(shared_bias), _p(shared_noise), _p(karena), karena.stride(1), karena.stride(0),
                                        _p(ws_arena), ws_arena.stride(0), _p(info), _p(rows), ldr, _p(z), _p(alpha), _p(bias),
                                        _p(noise), _p(scratch), _stream()), "cimrgp_layer_fit_cov")


def _w_work(batch, ns, ldw, like):
    """The W work area of a layer call: ``batch`` blocks of ``ns`` rows of pitch ``ldw``, allocated for that call only."""
    return torch.empty((batch, max(int(ns), 1), ldw), dtype=like.dtype, device=like.device)


def layer_predict(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, z, bias, noise, mean, var, cov=_lib.COV_RBF):
    """Predictive mean and variance of ``batch`` equal-sized blocks at ``ns`` test points each in ONE call
    (cimrgp_layer_predict_cov): accumulates into mean (N* x q) / var (N*,) at rows t_starts[b] ...; ``noise``
    (batch,) or None is added to the variance."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(larena.shape[0])
    ldw = padded_ld(n)
    w = _w_work(batch, ns, ldw, x)
    _lib.check(lib.cimrgp_layer_predict_cov(_DT[x.dtype], cov, _p(x), _p(starts), int(n), int(x.shape[1]), _p(xs), _p(t_starts),
                                            int(ns), batch, float(ell), float(sf2), _p(larena), larena.stride(1),
                                            larena.stride(0), _p(ws_arena), ws_arena.stride(0), _p(z), int(z.shape[2]), _p(bias),
                                            _p(noise), _p(w), ldw, w.stride(0), _p(mean), _p(var), _stream()),
               "cimrgp_layer_predict_cov")


def joint_ld(cols, dtype):
    """padded_ld, and at least 128 bytes: the row pitch of the joint calls' matrix-core operands."""
    return max(padded_ld(cols), 128 // torch.empty((), dtype=dtype).element_size())


def normal_fill(seed, keys, col0, cols, ns, z):
    """Standard normals phi(seed, keys[b], col0 + c, i) into z (batch, >= cols, ldz): row c of block b holds sample
    column col0 + c at points i < ns (cimrgp_normal_fill, include/cimrgp_joint.h).  keys: device int64 (batch,)."""
    lib = _lib.load()
    batch = int(z.shape[0])
    _lib.check(lib.cimrgp_normal_fill(_DT[z.dtype], int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keys), batch, int(col0), int(cols), int(ns),
                                      _p(z), z.stride(1), z.stride(0), _stream()), "cimrgp_normal_fill")
    return z


def layer_joint_cov(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, diag, carena, cws_arena=None, info=None,
                    cov=_lib.COV_RBF):
    """Predictive covariance blocks of ``batch`` equal-sized blocks in ONE call (cimrgp_layer_joint_cov): lower(carena[b])
    = K(xs_b, xs_b) + diag[b] I - W_b W_b^T, addressed as for :func:`layer_predict`; with ``cws_arena`` (batch, ws_bytes)
    uint8 and ``info`` (batch,) int32 each block is factored in place and its strict upper triangle zeroed.  diag:
    device (batch,) of the dtype, or None.  The W work area is allocated for this call only."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(larena.shape[0])
    ldw = joint_ld(n, x.dtype)
    w = _w_work(batch, ns, ldw, x)
    _lib.check(lib.cimrgp_layer_joint_cov(_DT[x.dtype], cov, _p(x), _p(starts), int(n), int(x.shape[1]), _p(xs), _p(t_starts),
                                          int(ns), batch, float(ell), float(sf2), _p(larena), larena.stride(1), larena.stride(0),
                                          _p(ws_arena), ws_arena.stride(0), _p(diag), _p(w), ldw, w.stride(0), _p(carena),
                                          carena.stride(1), carena.stride(0), _p(cws_arena),
                                          0 if cws_arena is None else cws_arena.stride(0), _p(info), _stream()),
               "cimrgp_layer_joint_cov")
    return carena


def layer_sample(larena, ns, z, cols, t_starts, out):
    """out[c, t_starts[b] + i] += sum_{k <= i} L_b[i, k] z[b, c, k] for c < cols (cimrgp_layer_sample): larena
    (batch, >= ns, ldl) factors, z (batch, >= cols, ldz) normals, out (cols, ld_out) shared by the blocks."""
    lib = _lib.load()
    batch = int(larena.shape[0])
    _lib.check(lib.cimrgp_layer_sample(_DT[larena.dtype], _p(larena), larena.stride(1), larena.stride(0), int(ns), batch, _p(z),
                                       z.stride(1), z.stride(0), int(cols), _p(t_starts), _p(out), out.stride(0), _stream()),
               "cimrgp_layer_sample")
    return out


def trsm_rows_lt(lbuf, n, ws, bbuf, m):
    """B <- B L^-1 on bbuf[:m, :n] (cimrgp_trsm_rows_lt, include/cimrgp_grad.h): after :func:`trsm_rows` the rows of
    K(X*, X) K^-1."""
    lib = _lib.load()
    _lib.check(lib.cimrgp_trsm_rows_lt(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), _p(bbuf), int(m),
                                       bbuf.stride(0), _stream()), "cimrgp_trsm_rows_lt")
    return bbuf


def trsm_rows_lt_batched(larena, n, ws_arena, barena, m):
    """B_b <- B_b L_b^-1 for every block b of larena (batch, >= n, ldl), ws_arena (batch, ws_bytes) uint8 and barena
    (batch, >= m, ldb) (cimrgp_trsm_rows_lt_batched)."""
    lib = _lib.load()
    batch = int(larena.shape[0])
    _lib.check(lib.cimrgp_trsm_rows_lt_batched(_DT[larena.dtype], _p(larena), int(n), larena.stride(1), larena.stride(0),
                                               _p(ws_arena), ws_arena.stride(0), _p(barena), int(m), barena.stride(1),
                                               barena.stride(0), batch, _stream()), "cimrgp_trsm_rows_lt_batched")
    return barena


def cov_predict_grad(x, alpha, xs, ell, sf2, beta=None, mean_grad=None, var_grad=None, accumulate=False, cov=_lib.COV_RBF):
    """The fused derivative contraction of one block (cimrgp_cov_predict_grad): mean_grad (ns, d, q) (+)= d mean / d xs
    from alpha (n x q); var_grad (ns, d) (+)= d var / d xs from beta (ns rows of K(xs, x) K^-1).  Either output may be
    None."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    n, d = x.shape
    q = int(alpha.shape[1]) if alpha is not None else int(mean_grad.shape[2]) if mean_grad is not None else 1
    ldb = beta.stride(0) if beta is not None else 0
    _lib.check(lib.cimrgp_cov_predict_grad(_DT[x.dtype], cov, _p(x), int(n), int(d), _p(alpha), q, _p(xs), int(xs.shape[0]),
                                           float(ell), float(sf2), _p(beta), ldb, _p(mean_grad), _p(var_grad),
                                           1 if accumulate else 0, _stream()), "cimrgp_cov_predict_grad")


def layer_predict_grad(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, alpha, mean_grad, var_grad,
                       cov=_lib.COV_RBF):
    """Predictive gradients of ``batch`` equal-sized blocks at ``ns`` test points each in ONE call
    (cimrgp_layer_predict_grad_cov): accumulates into mean_grad (N*, d, q) / var_grad (N*, d) at rows t_starts[b] ...;
    alpha (batch, n, q) contiguous.  The W work area is allocated for this call only (not without var_grad)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(larena.shape[0])
    ldw = padded_ld(n)
    w = _w_work(batch, ns, ldw, x) if var_grad is not None else None
    _lib.check(lib.cimrgp_layer_predict_grad_cov(_DT[x.dtype], cov, _p(x), _p(starts), int(n), int(x.shape[1]), _p(xs),
                                                 _p(t_starts), int(ns), batch, float(ell), float(sf2), _p(larena),
                                                 larena.stride(1), larena.stride(0), _p(ws_arena), ws_arena.stride(0),
                                                 _p(alpha), int(alpha.shape[2]), _p(w), ldw, 0 if w is None else w.stride(0),
                                                 _p(mean_grad), _p(var_grad), 1, _stream()),
               "cimrgp_layer_predict_grad_cov")


def trtri_rows(lbuf, n, ws, r0, m, out=None):
    """Rows [r0, r0 + m) of L^-T (cimrgp_trtri_rows, include/cimrgp_loo.h) into ``out`` (>= m rows of >= n columns, columns
    indexed as in L^-T; allocated with a padded pitch if None).  Columns left of r0 are neither read nor written."""
    lib = _lib.load()
    if out is None:
        out = alloc_matrix(m, n, lbuf.dtype, lbuf.device)
    _lib.check(lib.cimrgp_trtri_rows(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), int(r0), int(m), _p(out),
                                     out.stride(0), _stream()), "cimrgp_trtri_rows")
    return out


def kinv_diag_scratch_bytes(n, strip_rows, dtype):
    return int(_lib.load().cimrgp_kinv_diag_scratch_bytes(_DT[dtype], int(n), int(strip_rows)))


def kinv_diag(lbuf, n, ws, scratch_bytes, out=None):
    """diag(K^-1) of one factored block (cimrgp_kinv_diag), through a scratch of at most ``scratch_bytes`` bytes (at least
    one strip of 256 rows); the result does not depend on the scratch size."""
    lib = _lib.load()
    dtype = lbuf.dtype
    nbytes = min(max(int(scratch_bytes), kinv_diag_scratch_bytes(n, 256, dtype)), kinv_diag_scratch_bytes(n, n, dtype))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=lbuf.device)
    if out is None:
        out = torch.empty(int(n), dtype=dtype, device=lbuf.device)
    _lib.check(lib.cimrgp_kinv_diag(_DT[dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), _p(scratch), nbytes, _p(out), _stream()),
               "cimrgp_kinv_diag")
    return out


def kinv_diag_batched(larena, n, ws_arena, scratch_bytes, out=None):
    """diag(K_b^-1) for every block b of larena (batch, >= n, ldl) and ws_arena (batch, ws_bytes) uint8
    (cimrgp_kinv_diag_batched): (batch, n).  The scratch (at most ``scratch_bytes``, at least one strip of 256 rows per
    block) is shared evenly by the blocks."""
    lib = _lib.load()
    dtype = larena.dtype
    batch = int(larena.shape[0])
    nbytes = min(max(int(scratch_bytes), batch * kinv_diag_scratch_bytes(n, 256, dtype)), batch * kinv_diag_scratch_bytes(n, n, dtype))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=larena.device)
    if out is None:
        out = torch.empty((batch, int(n)), dtype=dtype, device=larena.device)
    _lib.check(lib.cimrgp_kinv_diag_batched(_DT[dtype], _p(larena), int(n), larena.stride(1), larena.stride(0), _p(ws_arena),
                                            ws_arena.stride(0), _p(scratch), nbytes, _p(out), batch, _stream()),
               "cimrgp_kinv_diag_batched")
    return out


def loo(y, alpha, diag, mean_out=None, var_out=None, starts=None):
    """The leave-one-out tail (cimrgp_loo): mean_out = y - alpha / diag[:, None], var_out = 1 / diag; either may be None.
    With ``starts`` (batch,) int64 the batched form (cimrgp_loo_batched): alpha (batch, n, q), diag (batch, n), block b's
    rows of y, mean_out and var_out start at row starts[b]."""
    lib = _lib.load()
    q = int(alpha.shape[-1])
    if starts is None:
        _lib.check(lib.cimrgp_loo(_DT[diag.dtype], _p(y), _p(alpha), _p(diag), int(diag.shape[0]), q, _p(mean_out), _p(var_out),
                                  _stream()), "cimrgp_loo")
    else:
        _lib.check(lib.cimrgp_loo_batched(_DT[diag.dtype], _p(y), _p(starts), _p(alpha), _p(diag), int(diag.shape[1]), q,
                                          int(diag.shape[0]), _p(mean_out), _p(var_out), _stream()), "cimrgp_loo_batched")


def wsyrk_tn_scratch_bytes(n, m, q, dtype):
    return int(_lib.load().cimrgp_wsyrk_tn_scratch_bytes(_DT[dtype], int(n), int(m), int(q)))


def wsyrk_tn(abuf, n, m, w, r=None, diag_add=0.0, out=None, g=None, scratch=None):
    """lower(out)[:m, :m] = diag_add I + A^T diag(w) A and, with ``r`` (n x q), g (m x q) = A^T diag(w) r, for
    A = abuf[:n, :m] (cimrgp_wsyrk_tn, include/cimrgp_sparse.h).  Returns (out, g); out is allocated with a padded
    pitch if None, the scratch for this call only if None."""
    lib = _lib.load()
    dtype = abuf.dtype
    q = 0 if r is None else int(r.shape[1])
    if out is None:
        out = alloc_matrix(m, m, dtype, abuf.device)
    if r is not None and g is None:
        g = torch.empty((int(m), q), dtype=dtype, device=abuf.device)
    nbytes = wsyrk_tn_scratch_bytes(n, m, q, dtype)
    if scratch is None:
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=abuf.device)
    _lib.check(lib.cimrgp_wsyrk_tn(_DT[dtype], _p(abuf), int(n), int(m), abuf.stride(0), _p(w), _p(r), q, float(diag_add), _p(out),
                                   out.stride(0), _p(g), _p(scratch), scratch.numel(), _stream()), "cimrgp_wsyrk_tn")
    return out, g


def sparse_lambda(abuf, n, m, sf2, noise, mode, lam=None, w=None, sums=None):
    """lam, w = 1 / lam (n,) and sums = [sum log lam, sum (sf2 - q_i), #(lam <= 0)] (device float64[3]) from one pass
    over A = abuf[:n, :m] (cimrgp_sparse_lambda); mode 0: FITC, 1: VFE."""
    lib = _lib.load()
    if lam is None:
        lam = torch.empty(int(n), dtype=abuf.dtype, device=abuf.device)
    if w is None:
        w = torch.empty(int(n), dtype=abuf.dtype, device=abuf.device)
    if sums is None:
        sums = torch.empty(3, dtype=torch.float64, device=abuf.device)
    _lib.check(lib.cimrgp_sparse_lambda(_DT[abuf.dtype], _p(abuf), int(n), int(m), abuf.stride(0), float(sf2), float(noise), int(mode),
                                        _p(lam), _p(w), _p(sums), _stream()), "cimrgp_sparse_lambda")
    return lam, w, sums


def sparse_tail(astar, wstar, ns, m, gamma, sf2, extra_var=0.0, mean_out=None, var_out=None, accumulate=False):
    """mean_out (ns x q) (+)= W* gamma, var_out (ns) (+)= sf2 + extra_var - sum A*^2 + sum W*^2 (cimrgp_sparse_tail);
    either output may be None.  astar and wstar share their pitch."""
    lib = _lib.load()
    if astar is not None and astar.stride(0) != wstar.stride(0):
        raise ValueError("astar and wstar must have the same row pitch")
    q = 0 if gamma is None else int(gamma.shape[1])
    _lib.check(lib.cimrgp_sparse_tail(_DT[wstar.dtype], _p(astar), _p(wstar), int(ns), int(m), wstar.stride(0), _p(gamma), q,
                                      float(sf2), float(extra_var), _p(mean_out), _p(var_out), int(bool(accumulate)), _stream()),
               "cimrgp_sparse_tail")


def sparse_lambda_dev(abuf, n, m, sf2, noise_dev, mode, lam=None, w=None, sums=None):
    """:func:`sparse_lambda` with the noise variance a device scalar ``noise_dev`` (one element of abuf's dtype), read by
    the kernel: nothing comes back to the host (cimrgp_sparse_lambda_dev, include/cimrgp_sparse_layer.h)."""
    lib = _lib.load()
    if noise_dev.dtype != abuf.dtype or noise_dev.numel() < 1:
        raise ValueError("noise_dev must hold one element of the matrix's dtype")
    if lam is None:
        lam = torch.empty(int(n), dtype=abuf.dtype, device=abuf.device)
    if w is None:
        w = torch.empty(int(n), dtype=abuf.dtype, device=abuf.device)
    if sums is None:
        sums = torch.empty(3, dtype=torch.float64, device=abuf.device)
    _lib.check(lib.cimrgp_sparse_lambda_dev(_DT[abuf.dtype], _p(abuf), int(n), int(m), abuf.stride(0), float(sf2), _p(noise_dev),
                                            int(mode), _p(lam), _p(w), _p(sums), _stream()), "cimrgp_sparse_lambda_dev")
    return lam, w, sums


def sparse_tail_dev(astar, wstar, ns, m, gamma, sf2, extra_var=0.0, bias=None, extra_var_dev=None, mean_out=None, var_out=None,
                    accumulate=False):
    """:func:`sparse_tail` with a device bias (q,) added to every row of the mean and a device scalar ``extra_var_dev``
    added to the variance, either None (cimrgp_sparse_tail_dev, include/cimrgp_sparse_layer.h)."""
    lib = _lib.load()
    if astar is not None and astar.stride(0) != wstar.stride(0):
        raise ValueError("astar and wstar must have the same row pitch")
    q = 0 if gamma is None else int(gamma.shape[1])
    if bias is not None and (bias.dtype != wstar.dtype or bias.numel() < q):
        raise ValueError("bias must hold q elements of the matrices' dtype")
    if extra_var_dev is not None and (extra_var_dev.dtype != wstar.dtype or extra_var_dev.numel() < 1):
        raise ValueError("extra_var_dev must hold one element of the matrices' dtype")
    _lib.check(lib.cimrgp_sparse_tail_dev(_DT[wstar.dtype], _p(astar), _p(wstar), int(ns), int(m), wstar.stride(0), _p(gamma), q,
                                          float(sf2), float(extra_var), _p(bias), _p(extra_var_dev), _p(mean_out), _p(var_out),
                                          int(bool(accumulate)), _stream()), "cimrgp_sparse_tail_dev")


def cov_pair_grad_scratch_bytes(na, nb, d):
    return int(_lib.load().cimrgp_cov_pair_grad_scratch_bytes(int(na), int(nb), int(d)))


def cov_pair_grad_ard_scratch_bytes(na, nb, d):
    return int(_lib.load().cimrgp_cov_pair_grad_ard_scratch_bytes(int(na), int(nb), int(d)))


def _pair_grad(name, nsums, scratch_bytes, xa, xb, gbuf, ell, sf2, scale, accumulate, sums, db, want_sums, want_db, cov, scratch):
    """The one call of the two pair contractions: the C function ``name`` with ``nsums`` scalar sums."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    na, d = xa.shape
    nb = xb.shape[0]
    if want_sums and sums is None:
        sums = torch.zeros(nsums, dtype=torch.float64, device=xa.device)
    if want_db and db is None:
        db = torch.zeros((int(nb), int(d)), dtype=xa.dtype, device=xa.device)
    nbytes = scratch_bytes(na, nb, d)
    if scratch is None:
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xa.device)
    _lib.check(getattr(lib, name)(_DT[xa.dtype], cov, _p(xa), int(na), _p(xb), int(nb), int(d), _p(gbuf), gbuf.stride(0),
                                  float(ell), float(sf2), float(scale), int(bool(accumulate)), _p(sums if want_sums else None),
                                  _p(db if want_db else None), _p(scratch), scratch.numel(), _stream()), name)
    return sums, db


def cov_pair_grad(xa, xb, gbuf, ell, sf2, scale=1.0, accumulate=False, sums=None, db=None, want_sums=True, want_db=True,
                  cov=_lib.COV_RBF, scratch=None):
    """sums (device float64[2]) (+)= [sum G o K, sum G o dK/dlog l] and db (nb x d) (+)= scale sum_i G_ij g(r_ij) (xa_i - xb_j)
    for G = gbuf[:na, :nb] and the pairs (xa_i, xb_j) (cimrgp_cov_pair_grad, include/cimrgp_sparse_grad.h).  Returns
    (sums, db); an output that is wanted and not given is allocated, the scratch for this call only if None."""
    return _pair_grad("cimrgp_cov_pair_grad", 2, cov_pair_grad_scratch_bytes, xa, xb, gbuf, ell, sf2, scale, accumulate, sums, db,
                      want_sums, want_db, cov, scratch)


def cov_pair_grad_ard(xa, xb, gbuf, ell, sf2, scale=1.0, accumulate=False, sums=None, db=None, want_sums=True, want_db=True,
                      cov=_lib.COV_RBF, scratch=None):
    """The ARD twin of :func:`cov_pair_grad`: sums (device float64[1 + d]) (+)= [sum G o K, sum G g (xa_e - xb_e)^2 for
    e = 0 .. d - 1], db as there (cimrgp_cov_pair_grad_ard, include/cimrgp_sparse_ard.h).  Returns (sums, db)."""
    return _pair_grad("cimrgp_cov_pair_grad_ard", 1 + int(xa.shape[1]), cov_pair_grad_ard_scratch_bytes, xa, xb, gbuf, ell, sf2,
                      scale, accumulate, sums, db, want_sums, want_db, cov, scratch)


def sparse_grad_rows(vbuf, n, m, gamma, r, w, mode, noise, beta=None, t=None, sums=None):
    """beta (n x q), t (n) and sums = [sum h_i, sum t_i] (device float64[2]) from one pass over V = vbuf[:n, :m]
    (cimrgp_sparse_grad_rows); mode 0: FITC, 1: VFE."""
    lib = _lib.load()
    q = int(gamma.shape[1])
    if beta is None:
        beta = torch.empty((int(n), q), dtype=vbuf.dtype, device=vbuf.device)
    if t is None:
        t = torch.empty(int(n), dtype=vbuf.dtype, device=vbuf.device)
    if sums is None:
        sums = torch.empty(2, dtype=torch.float64, device=vbuf.device)
    _lib.check(lib.cimrgp_sparse_grad_rows(_DT[vbuf.dtype], _p(vbuf), int(n), int(m), vbuf.stride(0), _p(gamma), _p(r), _p(w), q,
                                           int(mode), float(noise), _p(beta), _p(t), _p(sums), _stream()), "cimrgp_sparse_grad_rows")
    return beta, t, sums


def sparse_grad_combine(abuf, ybuf, n, m, beta, b, w, t):
    """ybuf[:n, :m] <- beta b^T - q diag(w) Y - 2 diag(t) A in place (cimrgp_sparse_grad_combine)."""
    lib = _lib.load()
    _lib.check(lib.cimrgp_sparse_grad_combine(_DT[abuf.dtype], _p(abuf), abuf.stride(0), _p(ybuf), ybuf.stride(0), int(n), int(m),
                                              _p(beta), _p(b), _p(w), _p(t), int(beta.shape[1]), _stream()),
               "cimrgp_sparse_grad_combine")
    return ybuf


def cov_cross_grad(xa, xb, ell, sf2, out, cov=_lib.COV_RBF):
    """The d + 1 slabs [K(xa, xb); dK / d xa_0; ..; dK / d xa_{d-1}] into ``out`` (d + 1, >= na, ldo) from one pass over
    the pairs (cimrgp_cov_cross_grad, include/cimrgp_sparse_post.h); slab 0 is :func:`rbf_cross`'s output bit for bit."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    na, d = xa.shape
    if out.dim() != 3 or int(out.shape[0]) != int(d) + 1 or int(out.shape[1]) < int(na) or out.stride(2) != 1:
        raise ValueError("out must be (d + 1, >= na, ldo) with unit column stride")
    _lib.check(lib.cimrgp_cov_cross_grad(_DT[xa.dtype], cov, _p(xa), int(na), _p(xb), int(xb.shape[0]), int(d), float(ell),
                                         float(sf2), _p(out), out.stride(1), out.stride(0), _stream()), "cimrgp_cov_cross_grad")
    return out


def sparse_tail_grad(aslabs, wslabs, ns, m, gamma, mean_grad=None, var_grad=None, accumulate=False):
    """mean_grad (ns, d, q) (+)= dW_e gamma and var_grad (ns, d) (+)= 2 sum_j (W* dW_e - A* dA_e) from the solved slabs
    ``aslabs`` / ``wslabs`` (d + 1, >= ns, ld), which share their layout (cimrgp_sparse_tail_grad); either output, and
    ``aslabs`` without ``var_grad``, may be None."""
    lib = _lib.load()
    if aslabs is not None and (aslabs.stride(0) != wslabs.stride(0) or aslabs.stride(1) != wslabs.stride(1)):
        raise ValueError("aslabs and wslabs must have the same row pitch and slab stride")
    q = 0 if gamma is None else int(gamma.shape[1])
    _lib.check(lib.cimrgp_sparse_tail_grad(_DT[wslabs.dtype], _p(aslabs), _p(wslabs), int(ns), int(m), int(wslabs.shape[0]) - 1,
                                           wslabs.stride(1), wslabs.stride(0), _p(gamma), q, _p(mean_grad), _p(var_grad),
                                           int(bool(accumulate)), _stream()), "cimrgp_sparse_tail_grad")


def sparse_loo(abuf, vbuf, n, m, gamma, r, sf2, noise, mode, bad, mean_out=None, var_out=None):
    """Leave-one-out mean (n x q) and variance (n,) of the rows of a sparse fit from A = abuf[:n, :m] and V = vbuf[:n, :m]
    (cimrgp_sparse_loo); ``bad`` (device int32[1]) counts the rows with 1 - h_i <= 0 and is never reset here."""
    lib = _lib.load()
    if abuf.stride(0) != vbuf.stride(0):
        raise ValueError("abuf and vbuf must have the same row pitch")
    if bad.dtype != torch.int32 or bad.numel() < 1:
        raise ValueError("bad must hold one int32")
    _lib.check(lib.cimrgp_sparse_loo(_DT[abuf.dtype], _p(abuf), _p(vbuf), int(n), int(m), abuf.stride(0), _p(gamma), _p(r),
                                     int(gamma.shape[1]), float(sf2), float(noise), int(mode), _p(mean_out), _p(var_out), _p(bad),
                                     _stream()), "cimrgp_sparse_loo")


def sparse_joint_cov(xs, ell, sf2, diag, astar, wstar, m, cbuf, cws=None, info=None, cov=_lib.COV_RBF):
    """lower(cbuf[:ns, :ns]) = K(xs, xs) + diag I - A* A*^T + W* W*^T (cimrgp_sparse_joint_cov); with ``cws`` (uint8
    workspace) and ``info`` (int32[1]) the block is factored in place and its strict upper triangle zeroed."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    if astar.stride(0) != wstar.stride(0):
        raise ValueError("astar and wstar must have the same row pitch")
    ns, d = xs.shape
    _lib.check(lib.cimrgp_sparse_joint_cov(_DT[xs.dtype], cov, _p(xs), int(ns), int(d), float(ell), float(sf2), float(diag),
                                           _p(astar), _p(wstar), int(m), astar.stride(0), _p(cbuf), cbuf.stride(0), _p(cws),
                                           0 if cws is None else cws.numel(), _p(info), _stream()), "cimrgp_sparse_joint_cov")
    return cbuf


def layer_lml_scratch_bytes(n, q, batch, dtype):
    return int(_lib.load().cimrgp_layer_lml_grad_scratch_bytes(_DT[dtype], int(n), int(q), int(batch)))


def layer_lml_grad(x, y, fbar, starts, n, ell, sf2, noise, shared_bias, karena, kinv_arena, ws_arena, info, out,
                   cov=_lib.COV_RBF):
    """Log marginal likelihood and its gradient w.r.t. (log sf, log l, log noise) of ``batch`` equal-sized blocks of
    one layer in ONE call (cimrgp_layer_lml_grad_cov, include/cimrgp.h), addressed as for :func:`layer_fit`.
    Targets: y - fbar - bias, bias = ``shared_bias`` (q,) or each block's column means.  karena / kinv_arena
    (batch, n, ld) receive L and the lower triangle of K^-1, ws_arena (batch, ws_bytes) uint8, info (batch,) int32;
    out (batch, 4) float64 = [LML | gradient] per block (undefined where info != 0)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(karena.shape[0])
    q = int(y.shape[1])
    scratch = torch.empty(max(layer_lml_scratch_bytes(n, q, batch, y.dtype), 16), dtype=torch.uint8, device=y.device)
    _lib.check(lib.cimrgp_layer_lml_grad_cov(_DT[y.dtype], cov, _p(x), _p(y), _p(fbar), _p(starts), batch, int(n), int(x.shape[1]),
                                             q, float(ell), float(sf2), float(noise), _p(shared_bias), _p(karena), karena.stride(1),
                                             karena.stride(0), _p(kinv_arena), _p(ws_arena), ws_arena.stride(0), _p(info),
                                             _p(scratch), _p(out), _stream()), "cimrgp_layer_lml_grad_cov")
    return out


def layer_lml_ard_scratch_bytes(n, q, batch, dtype):
    return int(_lib.load().cimrgp_layer_lml_grad_ard_scratch_bytes(_DT[dtype], int(n), int(q), int(batch)))


def layer_lml_grad_ard(xs, y, fbar, starts, n, sf2, noise, shared_bias, karena, kinv_arena, ws_arena, info, out, cov=_lib.COV_RBF):
    """:func:`layer_lml_grad` with one length-scale per input dimension (cimrgp_layer_lml_grad_ard_cov,
    include/cimrgp_layer_ard.h): ``xs`` holds the inputs already divided by their length-scales and the covariance runs at
    unit length-scale.  out (batch, d + 3) float64 = [LML | d/dlog sf | d/dlog l_1 .. l_d | d/dlog noise] per block
    (undefined where info != 0)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    batch = int(karena.shape[0])
    q = int(y.shape[1])
    scratch = torch.empty(max(layer_lml_ard_scratch_bytes(n, q, batch, y.dtype), 16), dtype=torch.uint8, device=y.device)
    _lib.check(lib.cimrgp_layer_lml_grad_ard_cov(_DT[y.dtype], cov, _p(xs), _p(y), _p(fbar), _p(starts), batch, int(n),
                                                 int(xs.shape[1]), q, float(sf2), float(noise), _p(shared_bias), _p(karena),
                                                 karena.stride(1), karena.stride(0), _p(kinv_arena), _p(ws_arena),
                                                 ws_arena.stride(0), _p(info), _p(scratch), _p(out), _stream()),
               "cimrgp_layer_lml_grad_ard_cov")
    return out


def solve_lt(lbuf, n, ws, z):
    """Backward half of D3: z (n x q) = L^-1 R is overwritten with alpha = L^-T z."""
    lib = _lib.load()
    q = z.shape[1]
    scratch = torch.empty(2 * q * max(int(n), 1), dtype=lbuf.dtype, device=lbuf.device)
    _lib.check(lib.cimrgp_solve_lt(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), _p(z), q,
                                   _p(scratch), _stream()), "cimrgp_solve_lt")
    return z


#: include/cimrgp.h CIMRGP_INFO_WATCHDOG: the factorisation's schedule failed, not the matrix
INFO_WATCHDOG = 0x7fffffff


def is_watchdog(code):
    """``code``: an ``info`` word, possibly after a trip through a floating-point collective (float32 rounds
    2^31 - 1 up to 2^31; sums over ranks only grow)."""
    return float(code) >= float(INFO_WATCHDOG) - 128.0


def raise_if_not_pd(info):
    """LinAlgError is the exception the reference's PD guard keys on (SanityCheck.py:59-65); a schedule
    watchdog (CIMRGP_INFO_WATCHDOG) is NOT a numerical failure and must not be repaired as one: RuntimeError."""
    code = int(info.item()) if isinstance(info, torch.Tensor) else int(info)
    if is_watchdog(code):
        raise RuntimeError("cimrgp_potrf: schedule watchdog (a device-side wait inside the factorisation expired; "
                           "the result is undefined and the matrix was not judged)")
    if code != 0:
        raise np.linalg.LinAlgError("Matrix is not positive definite (leading minor of order %d)" % code)


def potrs(lbuf, n, ws, rhs, want_z=False):
    """D3: rhs (n x q) is overwritten with alpha.  Returns z = L^-1 rhs if asked."""
    lib = _lib.load()
    q = rhs.shape[1]
    scratch = torch.empty(2 * q * max(int(n), 1), dtype=lbuf.dtype, device=lbuf.device)
    z = torch.empty_like(rhs) if want_z else None
    _lib.check(lib.cimrgp_potrs(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), _p(rhs), q,
                                _p(z), _p(scratch), _stream()), "cimrgp_potrs")
    return z


def trsm_rows(lbuf, n, ws, bbuf, m):
    """B <- B L^-T on bbuf[:m, :n]."""
    lib = _lib.load()
    _lib.check(lib.cimrgp_trsm_rows(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(ws), _p(bbuf),
                                    int(m), bbuf.stride(0), _stream()), "cimrgp_trsm_rows")
    return bbuf


def predict_mean(x, alpha, xs, ell, sf2, bias=None, out=None, accumulate=False, cov=_lib.COV_RBF):
    """D4 fused mean: out (ns x q) (+)= bias + K(xs, x) alpha; ``cov`` as for :func:`rbf_gram`."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    n, d = x.shape
    ns = xs.shape[0]
    q = alpha.shape[1]
    if out is None:
        out = torch.empty((ns, q), dtype=x.dtype, device=x.device)
        accumulate = False
    _lib.check(lib.cimrgp_cov_predict_mean(_DT[x.dtype], cov, _p(x), n, d, _p(alpha), q, _p(xs), ns, float(ell),
                                           float(sf2), _p(bias), _p(out), int(bool(accumulate)), _stream()),
               "cimrgp_cov_predict_mean")
    return out


def predict_from_w(wbuf, ns, n, z, sf2, extra_var=0.0, bias=None, mean_out=None, var_out=None, accumulate=False,
                   extra_var_dev=None):
    """``extra_var``: host number; ``extra_var_dev``: device scalar (e.g. a block's noise) -- both are added."""
    lib = _lib.load()
    q = 0 if z is None else z.shape[1]
    _lib.check(lib.cimrgp_predict_from_w(_DT[wbuf.dtype], _p(wbuf), int(ns), int(n), wbuf.stride(0), _p(z), q,
                                         float(sf2), float(extra_var), _p(extra_var_dev), _p(bias), _p(mean_out),
                                         _p(var_out), int(bool(accumulate)), _stream()), "cimrgp_predict_from_w")


def block_stats(y, fbar, stats_out=None):
    lib = _lib.load()
    n, q = y.shape
    if stats_out is None:
        stats_out = torch.empty(q + 1, dtype=y.dtype, device=y.device)
    _lib.check(lib.cimrgp_block_stats(_DT[y.dtype], _p(y), _p(fbar), n, q, _p(stats_out), _stream()),
               "cimrgp_block_stats")
    return stats_out


def residual(y, fbar, bias, out=None):
    lib = _lib.load()
    n, q = y.shape
    if out is None:
        out = torch.empty_like(y)
    _lib.check(lib.cimrgp_residual(_DT[y.dtype], _p(y), _p(fbar), _p(bias), n, q, _p(out), _stream()),
               "cimrgp_residual")
    return out


def train_mean(r, alpha, bias, noise, out, accumulate=False):
    lib = _lib.load()
    n, q = r.shape
    _lib.check(lib.cimrgp_train_mean(_DT[r.dtype], _p(r), _p(alpha), _p(bias), _p(noise), n, q, _p(out),
                                     int(bool(accumulate)), _stream()), "cimrgp_train_mean")
    return out


def add_diag(kbuf, n, noise):
    lib = _lib.load()
    _lib.check(lib.cimrgp_add_diag(_DT[kbuf.dtype], _p(kbuf), int(n), kbuf.stride(0), _p(noise), _stream()),
               "cimrgp_add_diag")


def noise_from_stats(stats, q, frac, floor_value, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty(1, dtype=stats.dtype, device=stats.device)
    _lib.check(lib.cimrgp_noise_from_stats(_DT[stats.dtype], _p(stats), int(q), float(frac), float(floor_value),
                                           _p(out), _stream()), "cimrgp_noise_from_stats")
    return out


def logdet_half(lbuf, n):
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float64, device=lbuf.device)
    _lib.check(lib.cimrgp_logdet_half(_DT[lbuf.dtype], _p(lbuf), int(n), lbuf.stride(0), _p(out), _stream()),
               "cimrgp_logdet_half")
    return out


def syrk_lower(cbuf, abuf, n, k):
    """cbuf[:n,:n] (lower) -= abuf[:n,:k] abuf[:n,:k]^T."""
    lib = _lib.load()
    _lib.check(lib.cimrgp_syrk_lower(_DT[cbuf.dtype], _p(cbuf), cbuf.stride(0), _p(abuf), abuf.stride(0), int(n), int(k),
                                     _stream()), "cimrgp_syrk_lower")
    return cbuf


def lml_grad(x, kinv, n, alpha, ell, sf2, noise, cov=_lib.COV_RBF):
    """Gradient of the log marginal likelihood w.r.t. (log sf, log l, log noise): device float64[3]."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    scratch = torch.empty(max(lib.cimrgp_lml_grad_scratch_bytes(int(n)), 8) // 8, dtype=torch.float64, device=x.device)
    _lib.check(lib.cimrgp_cov_lml_grad(_DT[x.dtype], cov, _p(x), int(n), x.shape[1], _p(kinv), kinv.stride(0), _p(alpha),
                                       alpha.shape[1], float(ell), float(sf2), float(noise), _p(out), _p(scratch), _stream()),
               "cimrgp_cov_lml_grad")
    return out


def lml_grad_ard(x_scaled, kinv, n, alpha, sf2, noise, cov=_lib.COV_RBF):
    """ARD gradient w.r.t. (log sf, log l_1..l_d, log noise); ``x_scaled`` = inputs / length-scales."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    lib = _lib.load()
    d = x_scaled.shape[1]
    out = torch.empty(d + 2, dtype=torch.float64, device=x_scaled.device)
    scratch = torch.empty(max(lib.cimrgp_lml_grad_scratch_bytes(int(n)), 8) // 8, dtype=torch.float64, device=x_scaled.device)
    _lib.check(lib.cimrgp_cov_lml_grad_ard(_DT[x_scaled.dtype], cov, _p(x_scaled), int(n), d, _p(kinv), kinv.stride(0),
                                           _p(alpha), alpha.shape[1], float(sf2), float(noise), _p(out), _p(scratch),
                                           _stream()), "cimrgp_cov_lml_grad_ard")
    return out


# ---- reduced-rank (Laplacian basis) block path ------------------------------------------------
def _f64dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _interval_dev(interval, d, device):
    iv = _f64dev(np.asarray(interval, dtype=np.float64).reshape(-1), device)
    if iv.numel() != d:
        raise ValueError('Basis interval should have the same dimensionality as the input.')
    return iv


def laplace_basis(x, interval, n_basis, out=None):
    """Phi (n x m) of the Dirichlet-Laplacian eigenfunctions on [-L, L]^d for device points x."""
    n, d = x.shape
    if out is None:
        out = torch.empty((n, int(n_basis)), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    iv = _interval_dev(interval, d, x.device)
    if not x.is_contiguous():
        raise ValueError("laplace_basis needs contiguous inputs")
    _lib.check(lib.cimrgp_laplace_basis(_DT[x.dtype], _p(x), n, d, _p(iv), int(n_basis), _p(out), _stream()),
               "cimrgp_laplace_basis")
    return out


class BlockMoments(object):
    """Host copy of the sums one block's updates need (see include/cimrgp.h, cimrgp_basis_moments)."""
    __slots__ = ("proj", "colsum", "colsum2", "resid_sum", "resid_sq", "fvar_sum", "n")

    def __init__(self, rec, m, q, n):
        self.proj = rec[:m * q].reshape(m, q)           # Phi^T r0
        self.colsum = rec[m * q:m * q + m]
        self.colsum2 = rec[m * q + m:m * q + 2 * m]
        self.resid_sum = rec[m * q + 2 * m:m * q + 2 * m + q]
        self.resid_sq = float(rec[m * q + 2 * m + q])
        self.fvar_sum = float(rec[m * q + 2 * m + q + 1])
        self.n = int(n)


def basis_moments(x, interval, n_basis, y, fbar, fvar, eau):
    """Every N-dependent sum of one block's variational updates in one pass over the block's
    points, with r0 = y - fbar - Phi E[au]^T; Phi is regenerated from ``x`` (n x d, device) and
    the interval, never read.  ``eau``: (q x m) host array.  Returns BlockMoments (host)."""
    n, d = x.shape
    m = int(n_basis)
    q = y.shape[1]
    lib = _lib.load()
    rec_len = m * q + 2 * m + q + 2
    out = torch.empty(rec_len, dtype=torch.float64, device=x.device)
    scratch = torch.empty(max(lib.cimrgp_basis_moments_scratch_bytes(n, m, q), 8) // 8, dtype=torch.float64,
                          device=x.device)
    e = _f64dev(eau, x.device)
    iv = _interval_dev(interval, d, x.device)
    for t in (x, y, fbar, fvar):
        if t is not None and not t.is_contiguous():
            raise ValueError("basis_moments needs contiguous operands")
    _lib.check(lib.cimrgp_basis_moments(_DT[x.dtype], _p(x), n, d, _p(iv), m, _p(y), _p(fbar), _p(fvar), _p(e), q, _p(out),
                                        _p(scratch), _stream()), "cimrgp_basis_moments")
    return BlockMoments(out.cpu().numpy(), m, q, n)


def basis_apply(x, interval, n_basis, eau, bias=None, c2=None, bias_var=0.0, mean=None, var=None, accumulate=False):
    """mean (+)= bias + Phi E[au]^T ;  var (+)= bias_var + Phi^2 c2, Phi regenerated from x."""
    n, d = x.shape
    q = np.asarray(eau).shape[0]
    lib = _lib.load()
    e = _f64dev(eau, x.device)
    b = None if bias is None else _f64dev(bias, x.device)
    c = None if c2 is None else _f64dev(c2, x.device)
    iv = _interval_dev(interval, d, x.device)
    for t in (x, mean, var):
        if t is not None and not t.is_contiguous():
            raise ValueError("basis_apply needs contiguous operands")
    _lib.check(lib.cimrgp_basis_apply(_DT[x.dtype], _p(x), n, d, _p(iv), int(n_basis), _p(e), q, _p(b), _p(c),
                                      float(bias_var), _p(mean), _p(var), int(bool(accumulate)), _stream()),
               "cimrgp_basis_apply")
