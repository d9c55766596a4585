"""Thin, typed wrappers around the C ABI operating on torch CUDA tensors.

torch is used for device memory, streams and (elsewhere) torch.distributed --
plumbing only; every arithmetic operation of the path below is a hand-written
HIP kernel reached through ``libcimrgp.so``.

Every wrapper reaches C through :func:`_call` (or :func:`_size` for the host-side size queries), which converts the
arguments by the ctypes signature registered in ``_lib`` ("The Python binding").
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
    """A tensor's address for a by-hand call of the library (tests/test_gpu_matern.py); the wrappers go through _call."""
    return None if t is None else t.data_ptr()


#: C function -> the Python function that marshals its wrapper's arguments, compiled at the wrapper's first call
_MARSHALLERS = {}
#: how an argument is written in that function, by registered argtype; every integer type is int(a)
_CONVERSIONS = {ctypes.c_void_p: "(None if {a} is None else {a}.data_ptr())", ctypes.c_double: "float({a})"}
_STATUS_CALL = "    rc = _lib.load().{name}({args})\n    if rc:\n        _lib.check(rc, '{name}')\n"
_SIZE_QUERY = "    return int(_lib.load().{name}({args}))\n"


def _marshaller(name, args, nstreams, body):
    """Compile the stanza a wrapper would otherwise write by hand, from ``name``'s registered argtypes -- for
    cimrgp_trsm_rows::

        def cimrgp_trsm_rows(a0, a1, a2, a3, a4, a5, a6, a7, s0):
            rc = _lib.load().cimrgp_trsm_rows(_DT[a0], <a1's address>, int(a2), int(a3), <a4's>, <a5's>, int(a6), int(a7), s0)
            if rc: <raise CimrgpError in the function's name>

    A pointer takes a tensor or None, an integer type goes through int() (bools become 0 / 1, NumPy integers pass), a double
    through float(); a wrapper that passes a ``torch.dtype`` first has the C function's dtype id there (KeyError for one the
    library does not have).  The ``nstreams`` trailing arguments are stream handles and pass as they are.  The types are
    decided here, once, not per call."""
    argtypes = _lib.signatures()[name][1]
    if len(args) + nstreams != len(argtypes):
        raise TypeError("%s takes %d arguments, %d given" % (name, len(argtypes), len(args) + nstreams))
    params = ["a%d" % i for i in range(len(args))]
    terms = [_CONVERSIONS.get(t, "int({a})").format(a=a) for a, t in zip(params, argtypes)]
    if isinstance(args[0], torch.dtype):
        terms[0] = "_DT[a0]"
    streams = ["s%d" % i for i in range(nstreams)]
    source = ("def {name}({params}):\n" + body).format(name=name, params=", ".join(params + streams), args=", ".join(terms + streams))
    scope = {}
    exec(source, globals(), scope)          # _lib and _DT are this module's, looked up at each call
    _MARSHALLERS[name] = scope[name]
    return scope[name]


def _call(name, *args, streams=None):
    """The C function ``name`` on the current stream (``streams``: on these handles instead, for an entry point that
    takes several); raises CimrgpError in its name if it refuses."""
    if streams is None:
        streams = (_stream(),)
    (_MARSHALLERS.get(name) or _marshaller(name, args, len(streams), _STATUS_CALL))(*args, *streams)


def _size(name, *args):
    """A host-side size query of the C ABI (no stream, no status)."""
    return (_MARSHALLERS.get(name) or _marshaller(name, args, 0, _SIZE_QUERY))(*args)


def _given(t, shape, like, dtype=None, zeros=False):
    """``t`` if the caller gave it, else a new tensor of ``shape`` on ``like``'s device, of its dtype unless ``dtype``."""
    if t is not None:
        return t
    return (torch.zeros if zeros else torch.empty)(tuple(int(s) for s in shape), dtype=dtype or like.dtype, device=like.device)


def _byte_scratch(nbytes, device, given=None):
    """``given``, or a uint8 work area of ``nbytes`` (never empty) for one call."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device) if given is None else given


def _solve_scratch(q, n, like, batch=()):
    """The work area of a backward solve with ``q`` right-hand sides (per block of ``batch``)."""
    return torch.empty(tuple(batch) + (2 * q * max(int(n), 1),), dtype=like.dtype, device=like.device)


def _same_pitch(a, b, names):
    if a is not None and a.stride(0) != b.stride(0):
        raise ValueError("%s must have the same row pitch" % names)


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
    _call("cimrgp_cov_gram", x.dtype, cov, x, n, d, ell, sf2, diag_add, out, out.stride(0), lower_only)
    return out


def rbf_cross(xa, xb, ell, sf2, out=None, cov=_lib.COV_RBF):
    """Cross-Gram (na x nb) into a padded buffer; ``cov`` as for :func:`rbf_gram`."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    nb = xb.shape[0]
    if out is None:
        out = alloc_matrix(na, nb, xa.dtype, xa.device)
    _call("cimrgp_cov_cross", xa.dtype, cov, xa, na, xb, nb, d, ell, sf2, out, out.stride(0))
    return out


def potrf_workspace_bytes(n, dtype):
    return _size("cimrgp_potrf_workspace_bytes", dtype, n)


def potrf_workspace(n, dtype, device):
    return _byte_scratch(potrf_workspace_bytes(n, dtype), device)


def _potrf(name, kbuf, n, ws, info, *rows):
    """The one call of the two factorisations; ``rows``: the carried rows' (buffer, count, pitch)."""
    if ws is None:
        ws = potrf_workspace(n, kbuf.dtype, kbuf.device)
    info = _given(info, (1,), kbuf, torch.int32, zeros=True)
    _call(name, kbuf.dtype, kbuf, n, kbuf.stride(0), ws, ws.numel(), info, *rows)
    return ws, info


def potrf(kbuf, n, ws=None, info=None):
    """D2 in place on kbuf[:n, :n] (lower).  Returns (ws, info) -- info is a
    device int32 scalar written asynchronously (LAPACK convention)."""
    return _potrf("cimrgp_potrf", kbuf, n, ws, info)


def potrf_rows(kbuf, n, bbuf, m, ws=None, info=None):
    """D2 with m carried rows: kbuf[:n,:n] = L L^T in place and bbuf[:m,:n] <- bbuf L^-T."""
    return _potrf("cimrgp_potrf_rows", kbuf, n, ws, info, bbuf, m, bbuf.stride(0))


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
    n, d = x.shape
    q = y.shape[1]
    ns = 0 if xs is None else xs.shape[0]
    if scratch is None:
        scratch = _solve_scratch(q, n, x)
    elif scratch.numel() < 2 * q * max(n, 1) or scratch.dtype != x.dtype:
        raise ValueError("scratch must hold 2 q n elements of the block's dtype")
    args = (x.dtype, x, n, d, y, q, xs, ns, ell, sf2, noise, kbuf, kbuf.stride(0), ws, ws.numel(), info, wbuf, wbuf.stride(0),
            alpha, z, scratch, mean, var, add_noise, accumulate)
    if streams is not None:
        _call("cimrgp_block_posterior_staged", *args, streams=[s.cuda_stream for s in streams])
    else:
        _call("cimrgp_block_posterior", *args)
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
    _call("cimrgp_potrf_rows_batched", karena.dtype, karena, n, ld, karena.stride(0), ws_arena, ws_arena.stride(0), info,
          barena, m, ldb, 0 if barena is None else barena.stride(0), karena.shape[0])


def solve_lt_batched(karena, n, ld, ws_arena, z):
    """Backward halves for a batch: z (batch, n, q) = L^-1 R is overwritten with alpha."""
    batch, _, q = z.shape
    scratch = _solve_scratch(q, n, karena, (batch,))
    _call("cimrgp_solve_lt_batched", karena.dtype, karena, n, ld, karena.stride(0), ws_arena, ws_arena.stride(0), z, q,
          scratch, batch)
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
        hit = (shape, rows, _solve_scratch(q, n, rows, (batch,)))
        _LAYER_WORK[key] = hit
    return hit[1], hit[2]


def layer_fit(x, y, fbar, train_out, starts, n, ell, sf2, noise_fixed, noise_frac, noise_floor, shared_bias, shared_noise,
              karena, ws_arena, info, bias, noise, z, alpha, cov=_lib.COV_RBF):
    """The fit of ``batch`` equal-sized blocks of one layer in ONE call (cimrgp_layer_fit_cov, include/cimrgp.h).
    x, y, fbar, train_out: the LAYER's arrays (N x d / N x q); starts: device int64 (batch,) row offsets.
    karena (batch, n, ld), ws_arena (batch, ws_bytes) uint8, info (batch,) int32, bias (batch, q), noise (batch,),
    z / alpha (batch, n, q) are filled.  noise_fixed < 0: from the statistics (or ``shared_noise``)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    batch = int(karena.shape[0])
    q = int(y.shape[1])
    ldr = padded_ld(n)
    rows, scratch = _layer_work_areas(batch, q, int(n), ldr, y.dtype, y.device)
    _call("cimrgp_layer_fit_cov", y.dtype, cov, x, y, fbar, train_out, starts, batch, n, x.shape[1], q, ell, sf2, noise_fixed,
          noise_frac, noise_floor, shared_bias, shared_noise, karena, karena.stride(1), karena.stride(0), ws_arena,
          ws_arena.stride(0), info, rows, ldr, z, alpha, bias, noise, scratch)


def _w_work(batch, ns, ldw, like):
    """The W work area of a layer call: ``batch`` blocks of ``ns`` rows of pitch ``ldw``, allocated for that call only."""
    return torch.empty((batch, max(int(ns), 1), ldw), dtype=like.dtype, device=like.device)


def layer_predict(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, z, bias, noise, mean, var, cov=_lib.COV_RBF):
    """Predictive mean and variance of ``batch`` equal-sized blocks at ``ns`` test points each in ONE call
    (cimrgp_layer_predict_cov): accumulates into mean (N* x q) / var (N*,) at rows t_starts[b] ...; ``noise``
    (batch,) or None is added to the variance."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    batch = int(larena.shape[0])
    ldw = padded_ld(n)
    w = _w_work(batch, ns, ldw, x)
    _call("cimrgp_layer_predict_cov", x.dtype, cov, x, starts, n, x.shape[1], xs, t_starts, ns, batch, ell, sf2, larena,
          larena.stride(1), larena.stride(0), ws_arena, ws_arena.stride(0), z, z.shape[2], bias, noise, w, ldw, w.stride(0),
          mean, var)


def joint_ld(cols, dtype):
    """padded_ld, and at least 128 bytes: the row pitch of the joint calls' matrix-core operands."""
    return max(padded_ld(cols), 128 // torch.empty((), dtype=dtype).element_size())


def normal_fill(seed, keys, col0, cols, ns, z):
    """Standard normals phi(seed, keys[b], col0 + c, i) into z (batch, >= cols, ldz): row c of block b holds sample
    column col0 + c at points i < ns (cimrgp_normal_fill, include/cimrgp_joint.h).  keys: device int64 (batch,)."""
    _call("cimrgp_normal_fill", z.dtype, int(seed) & 0xFFFFFFFFFFFFFFFF, keys, z.shape[0], col0, cols, ns, z, z.stride(1),
          z.stride(0))
    return z


def layer_joint_cov(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, diag, carena, cws_arena=None, info=None,
                    cov=_lib.COV_RBF):
    """Predictive covariance blocks of ``batch`` equal-sized blocks in ONE call (cimrgp_layer_joint_cov): lower(carena[b])
    = K(xs_b, xs_b) + diag[b] I - W_b W_b^T, addressed as for :func:`layer_predict`; with ``cws_arena`` (batch, ws_bytes)
    uint8 and ``info`` (batch,) int32 each block is factored in place and its strict upper triangle zeroed.  diag:
    device (batch,) of the dtype, or None.  The W work area is allocated for this call only."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    batch = int(larena.shape[0])
    ldw = joint_ld(n, x.dtype)
    w = _w_work(batch, ns, ldw, x)
    _call("cimrgp_layer_joint_cov", x.dtype, cov, x, starts, n, x.shape[1], xs, t_starts, ns, batch, ell, sf2, larena,
          larena.stride(1), larena.stride(0), ws_arena, ws_arena.stride(0), diag, w, ldw, w.stride(0), carena,
          carena.stride(1), carena.stride(0), cws_arena, 0 if cws_arena is None else cws_arena.stride(0), info)
    return carena


def layer_sample(larena, ns, z, cols, t_starts, out):
    """out[c, t_starts[b] + i] += sum_{k <= i} L_b[i, k] z[b, c, k] for c < cols (cimrgp_layer_sample): larena
    (batch, >= ns, ldl) factors, z (batch, >= cols, ldz) normals, out (cols, ld_out) shared by the blocks."""
    _call("cimrgp_layer_sample", larena.dtype, larena, larena.stride(1), larena.stride(0), ns, larena.shape[0], z, z.stride(1),
          z.stride(0), cols, t_starts, out, out.stride(0))
    return out


def trsm_rows_lt(lbuf, n, ws, bbuf, m):
    """B <- B L^-1 on bbuf[:m, :n] (cimrgp_trsm_rows_lt, include/cimrgp_grad.h): after :func:`trsm_rows` the rows of
    K(X*, X) K^-1."""
    _call("cimrgp_trsm_rows_lt", lbuf.dtype, lbuf, n, lbuf.stride(0), ws, bbuf, m, bbuf.stride(0))
    return bbuf


def trsm_rows_lt_batched(larena, n, ws_arena, barena, m):
    """B_b <- B_b L_b^-1 for every block b of larena (batch, >= n, ldl), ws_arena (batch, ws_bytes) uint8 and barena
    (batch, >= m, ldb) (cimrgp_trsm_rows_lt_batched)."""
    _call("cimrgp_trsm_rows_lt_batched", larena.dtype, larena, n, larena.stride(1), larena.stride(0), ws_arena,
          ws_arena.stride(0), barena, m, barena.stride(1), barena.stride(0), larena.shape[0])
    return barena


def cov_predict_grad(x, alpha, xs, ell, sf2, beta=None, mean_grad=None, var_grad=None, accumulate=False, cov=_lib.COV_RBF):
    """The fused derivative contraction of one block (cimrgp_cov_predict_grad): mean_grad (ns, d, q) (+)= d mean / d xs
    from alpha (n x q); var_grad (ns, d) (+)= d var / d xs from beta (ns rows of K(xs, x) K^-1).  Either output may be
    None."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    n, d = x.shape
    q = alpha.shape[1] if alpha is not None else mean_grad.shape[2] if mean_grad is not None else 1
    ldb = beta.stride(0) if beta is not None else 0
    _call("cimrgp_cov_predict_grad", x.dtype, cov, x, n, d, alpha, q, xs, xs.shape[0], ell, sf2, beta, ldb, mean_grad, var_grad,
          accumulate)


def layer_predict_grad(x, starts, n, xs, t_starts, ns, ell, sf2, larena, ws_arena, alpha, mean_grad, var_grad,
                       cov=_lib.COV_RBF):
    """Predictive gradients of ``batch`` equal-sized blocks at ``ns`` test points each in ONE call
    (cimrgp_layer_predict_grad_cov): accumulates into mean_grad (N*, d, q) / var_grad (N*, d) at rows t_starts[b] ...;
    alpha (batch, n, q) contiguous.  The W work area is allocated for this call only (not without var_grad)."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    batch = int(larena.shape[0])
    ldw = padded_ld(n)
    w = _w_work(batch, ns, ldw, x) if var_grad is not None else None
    _call("cimrgp_layer_predict_grad_cov", x.dtype, cov, x, starts, n, x.shape[1], xs, t_starts, ns, batch, ell, sf2, larena,
          larena.stride(1), larena.stride(0), ws_arena, ws_arena.stride(0), alpha, alpha.shape[2], w, ldw,
          0 if w is None else w.stride(0), mean_grad, var_grad, 1)          # 1: always accumulates


def trtri_rows(lbuf, n, ws, r0, m, out=None):
    """Rows [r0, r0 + m) of L^-T (cimrgp_trtri_rows, include/cimrgp_loo.h) into ``out`` (>= m rows of >= n columns, columns
    indexed as in L^-T; allocated with a padded pitch if None).  Columns left of r0 are neither read nor written."""
    if out is None:
        out = alloc_matrix(m, n, lbuf.dtype, lbuf.device)
    _call("cimrgp_trtri_rows", lbuf.dtype, lbuf, n, lbuf.stride(0), ws, r0, m, out, out.stride(0))
    return out


def kinv_diag_scratch_bytes(n, strip_rows, dtype):
    return _size("cimrgp_kinv_diag_scratch_bytes", dtype, n, strip_rows)


def _kinv_diag(name, blocks, lbuf, n, where, scratch_bytes, out, out_shape, *batch):
    """The one call of the two diag(K^-1): ``where`` is the factors' and workspaces' addressing, ``blocks`` how many share
    the scratch."""
    dtype = lbuf.dtype
    nbytes = min(max(int(scratch_bytes), blocks * kinv_diag_scratch_bytes(n, 256, dtype)),
                 blocks * kinv_diag_scratch_bytes(n, n, dtype))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=lbuf.device)
    out = _given(out, out_shape, lbuf)
    _call(name, dtype, lbuf, n, *where, scratch, nbytes, out, *batch)
    return out


def kinv_diag(lbuf, n, ws, scratch_bytes, out=None):
    """diag(K^-1) of one factored block (cimrgp_kinv_diag), through a scratch of at most ``scratch_bytes`` bytes (at least
    one strip of 256 rows); the result does not depend on the scratch size."""
    return _kinv_diag("cimrgp_kinv_diag", 1, lbuf, n, (lbuf.stride(0), ws), scratch_bytes, out, (n,))


def kinv_diag_batched(larena, n, ws_arena, scratch_bytes, out=None):
    """diag(K_b^-1) for every block b of larena (batch, >= n, ldl) and ws_arena (batch, ws_bytes) uint8
    (cimrgp_kinv_diag_batched): (batch, n).  The scratch (at most ``scratch_bytes``, at least one strip of 256 rows per
    block) is shared evenly by the blocks."""
    batch = int(larena.shape[0])
    return _kinv_diag("cimrgp_kinv_diag_batched", batch, larena, n, (larena.stride(1), larena.stride(0), ws_arena, ws_arena.stride(0)),
                      scratch_bytes, out, (batch, n), batch)


def loo(y, alpha, diag, mean_out=None, var_out=None, starts=None):
    """The leave-one-out tail (cimrgp_loo): mean_out = y - alpha / diag[:, None], var_out = 1 / diag; either may be None.
    With ``starts`` (batch,) int64 the batched form (cimrgp_loo_batched): alpha (batch, n, q), diag (batch, n), block b's
    rows of y, mean_out and var_out start at row starts[b]."""
    q = alpha.shape[-1]
    if starts is None:
        _call("cimrgp_loo", diag.dtype, y, alpha, diag, diag.shape[0], q, mean_out, var_out)
    else:
        _call("cimrgp_loo_batched", diag.dtype, y, starts, alpha, diag, diag.shape[1], q, diag.shape[0], mean_out, var_out)


def wsyrk_tn_scratch_bytes(n, m, q, dtype):
    return _size("cimrgp_wsyrk_tn_scratch_bytes", dtype, n, m, q)


def wsyrk_tn(abuf, n, m, w, r=None, diag_add=0.0, out=None, g=None, scratch=None):
    """lower(out)[:m, :m] = diag_add I + A^T diag(w) A and, with ``r`` (n x q), g (m x q) = A^T diag(w) r, for
    A = abuf[:n, :m] (cimrgp_wsyrk_tn, include/cimrgp_sparse.h).  Returns (out, g); out is allocated with a padded
    pitch if None, the scratch for this call only if None."""
    dtype = abuf.dtype
    q = 0 if r is None else int(r.shape[1])
    if out is None:
        out = alloc_matrix(m, m, dtype, abuf.device)
    if r is not None:
        g = _given(g, (m, q), abuf)
    scratch = _byte_scratch(wsyrk_tn_scratch_bytes(n, m, q, dtype), abuf.device, scratch)
    _call("cimrgp_wsyrk_tn", dtype, abuf, n, m, abuf.stride(0), w, r, q, diag_add, out, out.stride(0), g, scratch, scratch.numel())
    return out, g


def _sparse_lambda(name, abuf, n, m, sf2, noise, mode, lam, w, sums):
    """The one call of the two lambda passes; ``noise``: a host number or a device scalar, as ``name`` takes it."""
    lam, w = _given(lam, (n,), abuf), _given(w, (n,), abuf)
    sums = _given(sums, (3,), abuf, torch.float64)
    _call(name, abuf.dtype, abuf, n, m, abuf.stride(0), sf2, noise, mode, lam, w, sums)
    return lam, w, sums


def sparse_lambda(abuf, n, m, sf2, noise, mode, lam=None, w=None, sums=None):
    """lam, w = 1 / lam (n,) and sums = [sum log lam, sum (sf2 - q_i), #(lam <= 0)] (device float64[3]) from one pass
    over A = abuf[:n, :m] (cimrgp_sparse_lambda); mode 0: FITC, 1: VFE."""
    return _sparse_lambda("cimrgp_sparse_lambda", abuf, n, m, sf2, noise, mode, lam, w, sums)


def _sparse_tail(name, astar, wstar, ns, m, gamma, sf2, extra_var, dev_terms, mean_out, var_out, accumulate):
    """The one call of the two tails; ``dev_terms``: () or the device twin's (bias, extra_var_dev), checked here."""
    _same_pitch(astar, wstar, "astar and wstar")
    q = 0 if gamma is None else gamma.shape[1]
    for t, count, what in zip(dev_terms, (q, 1), ("bias must hold q elements", "extra_var_dev must hold one element")):
        if t is not None and (t.dtype != wstar.dtype or t.numel() < count):
            raise ValueError(what + " of the matrices' dtype")
    _call(name, wstar.dtype, astar, wstar, ns, m, wstar.stride(0), gamma, q, sf2, extra_var, *dev_terms, mean_out, var_out,
          accumulate)


def sparse_tail(astar, wstar, ns, m, gamma, sf2, extra_var=0.0, mean_out=None, var_out=None, accumulate=False):
    """mean_out (ns x q) (+)= W* gamma, var_out (ns) (+)= sf2 + extra_var - sum A*^2 + sum W*^2 (cimrgp_sparse_tail);
    either output may be None.  astar and wstar share their pitch."""
    _sparse_tail("cimrgp_sparse_tail", astar, wstar, ns, m, gamma, sf2, extra_var, (), mean_out, var_out, accumulate)


def sparse_lambda_dev(abuf, n, m, sf2, noise_dev, mode, lam=None, w=None, sums=None):
    """:func:`sparse_lambda` with the noise variance a device scalar ``noise_dev`` (one element of abuf's dtype), read by
    the kernel: nothing comes back to the host (cimrgp_sparse_lambda_dev, include/cimrgp_sparse_layer.h)."""
    if noise_dev.dtype != abuf.dtype or noise_dev.numel() < 1:
        raise ValueError("noise_dev must hold one element of the matrix's dtype")
    return _sparse_lambda("cimrgp_sparse_lambda_dev", abuf, n, m, sf2, noise_dev, mode, lam, w, sums)


def sparse_tail_dev(astar, wstar, ns, m, gamma, sf2, extra_var=0.0, bias=None, extra_var_dev=None, mean_out=None, var_out=None,
                    accumulate=False):
    """:func:`sparse_tail` with a device bias (q,) added to every row of the mean and a device scalar ``extra_var_dev``
    added to the variance, either None (cimrgp_sparse_tail_dev, include/cimrgp_sparse_layer.h)."""
    _sparse_tail("cimrgp_sparse_tail_dev", astar, wstar, ns, m, gamma, sf2, extra_var, (bias, extra_var_dev), mean_out, var_out,
                 accumulate)


def cov_pair_grad_scratch_bytes(na, nb, d):
    return _size("cimrgp_cov_pair_grad_scratch_bytes", na, nb, d)


def cov_pair_grad_ard_scratch_bytes(na, nb, d):
    return _size("cimrgp_cov_pair_grad_ard_scratch_bytes", na, nb, d)


def _pair_grad(name, nsums, scratch_bytes, xa, xb, gbuf, ell, sf2, scale, accumulate, sums, db, want_sums, want_db, cov, scratch):
    """The one call of the two pair contractions: the C function ``name`` with ``nsums`` scalar sums."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    nb = xb.shape[0]
    if want_sums:
        sums = _given(sums, (nsums,), xa, torch.float64, zeros=True)
    if want_db:
        db = _given(db, (nb, d), xa, zeros=True)
    scratch = _byte_scratch(scratch_bytes(na, nb, d), xa.device, scratch)
    _call(name, xa.dtype, cov, xa, na, xb, nb, d, gbuf, gbuf.stride(0), ell, sf2, scale, accumulate, sums if want_sums else None,
          db if want_db else None, scratch, scratch.numel())
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
    q = gamma.shape[1]
    beta, t = _given(beta, (n, q), vbuf), _given(t, (n,), vbuf)
    sums = _given(sums, (2,), vbuf, torch.float64)
    _call("cimrgp_sparse_grad_rows", vbuf.dtype, vbuf, n, m, vbuf.stride(0), gamma, r, w, q, mode, noise, beta, t, sums)
    return beta, t, sums


def sparse_grad_combine(abuf, ybuf, n, m, beta, b, w, t):
    """ybuf[:n, :m] <- beta b^T - q diag(w) Y - 2 diag(t) A in place (cimrgp_sparse_grad_combine)."""
    _call("cimrgp_sparse_grad_combine", abuf.dtype, abuf, abuf.stride(0), ybuf, ybuf.stride(0), n, m, beta, b, w, t, beta.shape[1])
    return ybuf


def cov_cross_grad(xa, xb, ell, sf2, out, cov=_lib.COV_RBF):
    """The d + 1 slabs [K(xa, xb); dK / d xa_0; ..; dK / d xa_{d-1}] into ``out`` (d + 1, >= na, ldo) from one pass over
    the pairs (cimrgp_cov_cross_grad, include/cimrgp_sparse_post.h); slab 0 is :func:`rbf_cross`'s output bit for bit."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    na, d = xa.shape
    if out.dim() != 3 or int(out.shape[0]) != int(d) + 1 or int(out.shape[1]) < int(na) or out.stride(2) != 1:
        raise ValueError("out must be (d + 1, >= na, ldo) with unit column stride")
    _call("cimrgp_cov_cross_grad", xa.dtype, cov, xa, na, xb, xb.shape[0], d, ell, sf2, out, out.stride(1), out.stride(0))
    return out


def sparse_tail_grad(aslabs, wslabs, ns, m, gamma, mean_grad=None, var_grad=None, accumulate=False):
    """mean_grad (ns, d, q) (+)= dW_e gamma and var_grad (ns, d) (+)= 2 sum_j (W* dW_e - A* dA_e) from the solved slabs
    ``aslabs`` / ``wslabs`` (d + 1, >= ns, ld), which share their layout (cimrgp_sparse_tail_grad); either output, and
    ``aslabs`` without ``var_grad``, may be None."""
    if aslabs is not None and (aslabs.stride(0) != wslabs.stride(0) or aslabs.stride(1) != wslabs.stride(1)):
        raise ValueError("aslabs and wslabs must have the same row pitch and slab stride")
    q = 0 if gamma is None else gamma.shape[1]
    _call("cimrgp_sparse_tail_grad", wslabs.dtype, aslabs, wslabs, ns, m, wslabs.shape[0] - 1, wslabs.stride(1), wslabs.stride(0),
          gamma, q, mean_grad, var_grad, accumulate)


def sparse_loo(abuf, vbuf, n, m, gamma, r, sf2, noise, mode, bad, mean_out=None, var_out=None):
    """Leave-one-out mean (n x q) and variance (n,) of the rows of a sparse fit from A = abuf[:n, :m] and V = vbuf[:n, :m]
    (cimrgp_sparse_loo); ``bad`` (device int32[1]) counts the rows with 1 - h_i <= 0 and is never reset here."""
    _same_pitch(abuf, vbuf, "abuf and vbuf")
    if bad.dtype != torch.int32 or bad.numel() < 1:
        raise ValueError("bad must hold one int32")
    _call("cimrgp_sparse_loo", abuf.dtype, abuf, vbuf, n, m, abuf.stride(0), gamma, r, gamma.shape[1], sf2, noise, mode, mean_out,
          var_out, bad)


def sparse_joint_cov(xs, ell, sf2, diag, astar, wstar, m, cbuf, cws=None, info=None, cov=_lib.COV_RBF):
    """lower(cbuf[:ns, :ns]) = K(xs, xs) + diag I - A* A*^T + W* W*^T (cimrgp_sparse_joint_cov); with ``cws`` (uint8
    workspace) and ``info`` (int32[1]) the block is factored in place and its strict upper triangle zeroed."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    _same_pitch(astar, wstar, "astar and wstar")
    ns, d = xs.shape
    _call("cimrgp_sparse_joint_cov", xs.dtype, cov, xs, ns, d, ell, sf2, diag, astar, wstar, m, astar.stride(0), cbuf,
          cbuf.stride(0), cws, 0 if cws is None else cws.numel(), info)
    return cbuf


def layer_lml_scratch_bytes(n, q, batch, dtype):
    return _size("cimrgp_layer_lml_grad_scratch_bytes", dtype, n, q, batch)


def _layer_lml_grad(name, scratch_bytes, x, y, fbar, starts, n, hyper, shared_bias, karena, kinv_arena, ws_arena, info, out, cov):
    """The one call of the two layer objectives; ``hyper``: the host hyper-parameters as ``name`` takes them."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    batch = int(karena.shape[0])
    q = int(y.shape[1])
    scratch = _byte_scratch(scratch_bytes(n, q, batch, y.dtype), y.device)
    _call(name, y.dtype, cov, x, y, fbar, starts, batch, n, x.shape[1], q, *hyper, shared_bias, karena, karena.stride(1),
          karena.stride(0), kinv_arena, ws_arena, ws_arena.stride(0), info, scratch, out)
    return out


def layer_lml_grad(x, y, fbar, starts, n, ell, sf2, noise, shared_bias, karena, kinv_arena, ws_arena, info, out,
                   cov=_lib.COV_RBF):
    """Log marginal likelihood and its gradient w.r.t. (log sf, log l, log noise) of ``batch`` equal-sized blocks of
    one layer in ONE call (cimrgp_layer_lml_grad_cov, include/cimrgp.h), addressed as for :func:`layer_fit`.
    Targets: y - fbar - bias, bias = ``shared_bias`` (q,) or each block's column means.  karena / kinv_arena
    (batch, n, ld) receive L and the lower triangle of K^-1, ws_arena (batch, ws_bytes) uint8, info (batch,) int32;
    out (batch, 4) float64 = [LML | gradient] per block (undefined where info != 0)."""
    return _layer_lml_grad("cimrgp_layer_lml_grad_cov", layer_lml_scratch_bytes, x, y, fbar, starts, n, (ell, sf2, noise),
                           shared_bias, karena, kinv_arena, ws_arena, info, out, cov)


def layer_lml_ard_scratch_bytes(n, q, batch, dtype):
    return _size("cimrgp_layer_lml_grad_ard_scratch_bytes", dtype, n, q, batch)


def layer_lml_grad_ard(xs, y, fbar, starts, n, sf2, noise, shared_bias, karena, kinv_arena, ws_arena, info, out, cov=_lib.COV_RBF):
    """:func:`layer_lml_grad` with one length-scale per input dimension (cimrgp_layer_lml_grad_ard_cov,
    include/cimrgp_layer_ard.h): ``xs`` holds the inputs already divided by their length-scales and the covariance runs at
    unit length-scale.  out (batch, d + 3) float64 = [LML | d/dlog sf | d/dlog l_1 .. l_d | d/dlog noise] per block
    (undefined where info != 0)."""
    return _layer_lml_grad("cimrgp_layer_lml_grad_ard_cov", layer_lml_ard_scratch_bytes, xs, y, fbar, starts, n, (sf2, noise),
                           shared_bias, karena, kinv_arena, ws_arena, info, out, cov)


def solve_lt(lbuf, n, ws, z):
    """Backward half of D3: z (n x q) = L^-1 R is overwritten with alpha = L^-T z."""
    q = z.shape[1]
    _call("cimrgp_solve_lt", lbuf.dtype, lbuf, n, lbuf.stride(0), ws, z, q, _solve_scratch(q, n, lbuf))
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
    q = rhs.shape[1]
    scratch = _solve_scratch(q, n, lbuf)
    z = torch.empty_like(rhs) if want_z else None
    _call("cimrgp_potrs", lbuf.dtype, lbuf, n, lbuf.stride(0), ws, rhs, q, z, scratch)
    return z


def trsm_rows(lbuf, n, ws, bbuf, m):
    """B <- B L^-T on bbuf[:m, :n]."""
    _call("cimrgp_trsm_rows", lbuf.dtype, lbuf, n, lbuf.stride(0), ws, bbuf, m, bbuf.stride(0))
    return bbuf


def predict_mean(x, alpha, xs, ell, sf2, bias=None, out=None, accumulate=False, cov=_lib.COV_RBF):
    """D4 fused mean: out (ns x q) (+)= bias + K(xs, x) alpha; ``cov`` as for :func:`rbf_gram`."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    n, d = x.shape
    ns = xs.shape[0]
    q = alpha.shape[1]
    if out is None:
        out = torch.empty((ns, q), dtype=x.dtype, device=x.device)
        accumulate = False
    _call("cimrgp_cov_predict_mean", x.dtype, cov, x, n, d, alpha, q, xs, ns, ell, sf2, bias, out, accumulate)
    return out


def predict_from_w(wbuf, ns, n, z, sf2, extra_var=0.0, bias=None, mean_out=None, var_out=None, accumulate=False,
                   extra_var_dev=None):
    """``extra_var``: host number; ``extra_var_dev``: device scalar (e.g. a block's noise) -- both are added."""
    q = 0 if z is None else z.shape[1]
    _call("cimrgp_predict_from_w", wbuf.dtype, wbuf, ns, n, wbuf.stride(0), z, q, sf2, extra_var, extra_var_dev, bias, mean_out,
          var_out, accumulate)


def block_stats(y, fbar, stats_out=None):
    n, q = y.shape
    stats_out = _given(stats_out, (q + 1,), y)
    _call("cimrgp_block_stats", y.dtype, y, fbar, n, q, stats_out)
    return stats_out


def residual(y, fbar, bias, out=None):
    n, q = y.shape
    if out is None:
        out = torch.empty_like(y)
    _call("cimrgp_residual", y.dtype, y, fbar, bias, n, q, out)
    return out


def train_mean(r, alpha, bias, noise, out, accumulate=False):
    n, q = r.shape
    _call("cimrgp_train_mean", r.dtype, r, alpha, bias, noise, n, q, out, accumulate)
    return out


def add_diag(kbuf, n, noise):
    _call("cimrgp_add_diag", kbuf.dtype, kbuf, n, kbuf.stride(0), noise)


def noise_from_stats(stats, q, frac, floor_value, out=None):
    out = _given(out, (1,), stats)
    _call("cimrgp_noise_from_stats", stats.dtype, stats, q, frac, floor_value, out)
    return out


def logdet_half(lbuf, n):
    out = torch.empty(1, dtype=torch.float64, device=lbuf.device)
    _call("cimrgp_logdet_half", lbuf.dtype, lbuf, n, lbuf.stride(0), out)
    return out


def syrk_lower(cbuf, abuf, n, k):
    """cbuf[:n,:n] (lower) -= abuf[:n,:k] abuf[:n,:k]^T."""
    _call("cimrgp_syrk_lower", cbuf.dtype, cbuf, cbuf.stride(0), abuf, abuf.stride(0), n, k)
    return cbuf


def _f64_scratch(nbytes, device):
    """A float64 work area of at least ``nbytes`` bytes' worth of whole elements, never empty."""
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def _lml_grad(name, nout, x, kinv, n, alpha, hyper, cov):
    """The one call of the two gradients: ``nout`` derivatives from the host hyper-parameters ``hyper``."""
    cov = _cov_id(cov)             # an unknown id is refused before any allocation
    out = torch.empty(nout, dtype=torch.float64, device=x.device)
    scratch = _f64_scratch(_size("cimrgp_lml_grad_scratch_bytes", n), x.device)
    _call(name, x.dtype, cov, x, n, x.shape[1], kinv, kinv.stride(0), alpha, alpha.shape[1], *hyper, out, scratch)
    return out


def lml_grad(x, kinv, n, alpha, ell, sf2, noise, cov=_lib.COV_RBF):
    """Gradient of the log marginal likelihood w.r.t. (log sf, log l, log noise): device float64[3]."""
    return _lml_grad("cimrgp_cov_lml_grad", 3, x, kinv, n, alpha, (ell, sf2, noise), cov)


def lml_grad_ard(x_scaled, kinv, n, alpha, sf2, noise, cov=_lib.COV_RBF):
    """ARD gradient w.r.t. (log sf, log l_1..l_d, log noise); ``x_scaled`` = inputs / length-scales."""
    return _lml_grad("cimrgp_cov_lml_grad_ard", x_scaled.shape[1] + 2, x_scaled, kinv, n, alpha, (sf2, noise), cov)


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
    out = _given(out, (n, n_basis), x)
    iv = _interval_dev(interval, d, x.device)
    if not x.is_contiguous():
        raise ValueError("laplace_basis needs contiguous inputs")
    _call("cimrgp_laplace_basis", x.dtype, x, n, d, iv, n_basis, out)
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
    rec_len = m * q + 2 * m + q + 2
    out = torch.empty(rec_len, dtype=torch.float64, device=x.device)
    scratch = _f64_scratch(_size("cimrgp_basis_moments_scratch_bytes", n, m, q), x.device)
    e = _f64dev(eau, x.device)
    iv = _interval_dev(interval, d, x.device)
    for t in (x, y, fbar, fvar):
        if t is not None and not t.is_contiguous():
            raise ValueError("basis_moments needs contiguous operands")
    _call("cimrgp_basis_moments", x.dtype, x, n, d, iv, m, y, fbar, fvar, e, q, out, scratch)
    return BlockMoments(out.cpu().numpy(), m, q, n)


def basis_apply(x, interval, n_basis, eau, bias=None, c2=None, bias_var=0.0, mean=None, var=None, accumulate=False):
    """mean (+)= bias + Phi E[au]^T ;  var (+)= bias_var + Phi^2 c2, Phi regenerated from x."""
    n, d = x.shape
    q = np.asarray(eau).shape[0]
    e = _f64dev(eau, x.device)
    b = None if bias is None else _f64dev(bias, x.device)
    c = None if c2 is None else _f64dev(c2, x.device)
    iv = _interval_dev(interval, d, x.device)
    for t in (x, mean, var):
        if t is not None and not t.is_contiguous():
            raise ValueError("basis_apply needs contiguous operands")
    _call("cimrgp_basis_apply", x.dtype, x, n, d, iv, n_basis, e, q, b, c, bias_var, mean, var, accumulate)
