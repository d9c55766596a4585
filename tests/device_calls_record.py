"""Every C call of cimrgp_amd/device.py, recorded on the CPU: shared by tests/test_device_calls_host.py, which replays
the cases below against the working tree's device.py and compares with tests/golden/device_calls.json.  Run as a script
(``python tests/device_calls_record.py``) it writes that file; the committed one was written from the commit before
device.py's calls went through one marshalling helper, and pins what reaches C across such rewrites.

How a wrapper is run without a GPU: the loaded library is replaced by a stand-in whose every function records
``[name, arguments]`` and returns 0 (the ``*_bytes`` size queries are host functions and are forwarded to the real
library, their result recorded too); ``device._stream`` returns a fixed handle; ``torch`` in device's namespace is a proxy
that records ``empty`` / ``zeros`` / ``empty_like`` / ``as_tensor``.  The operands are CPU tensors.

An event is ``["alloc", kind, shape, dtype, device]`` (``as_tensor``: plus the values) or ``[name, [argument, ...]]``
(size queries: plus the result), in the order they happen.  A scalar argument is recorded as itself -- JSON keeps int,
float and bool apart, and the comparison is made on the JSON text, so 1, 1.0 and true differ.  A pointer is recorded
as ``"<tensor>+<byte offset>"``: the case's name of the tensor whose storage it points into, ``#k`` for the wrapper's
k-th allocation, or a stream's name; null is ``null``.  A case also records what it returns (tensors by name, shape and
strides), the exception that ended it, and the keys and shapes of ``device._LAYER_WORK``.

Every case runs twice.  Variant 0: float32, contiguous or plainly padded operands, optional tensors omitted, flags off,
sizes as Python ints.  Variant 1: float64, every tensor a view at a nonzero offset into a larger buffer with a padded
pitch, optional tensors given, flags on, sizes as NumPy integers.  ``c.v`` is the variant."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cimrgp_amd import _lib, device as dev  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "device_calls.json")
STREAM = 0x5EED00           # the current stream's handle


class Stream(object):
    """What device.py reads of a torch stream."""

    def __init__(self, name, handle, device="gpu0"):
        self.name, self.cuda_stream, self.device = name, handle, device


class Recorder(object):
    def __init__(self):
        self.real = _lib.load()
        self.events = []
        self.named = []             # (name, tensor) of the case's operands
        self.allocs = []            # the wrapper's allocations, kept alive so that no address is used twice
        self.streams = {STREAM: "stream"}
        self.queue_out = None       # what cimrgp_solve_queue / cimrgp_front_queue write to *queue_out

    def alloc(self, kind, t, values=False):
        self.allocs.append(t)
        self.events.append(["alloc", kind, list(t.shape), str(t.dtype), str(t.device)] + ([t.tolist()] if values else []))
        return t

    def where(self, address):
        if address in self.streams:
            return self.streams[address]
        for label, t in self.named + [("#%d" % k, t) for k, t in enumerate(self.allocs)]:
            base = t.untyped_storage().data_ptr()
            if base <= address < base + max(t.untyped_storage().nbytes(), 1):
                return "%s+%d" % (label, address - base)
        raise AssertionError("pointer %#x belongs to no tensor of the case" % address)

    def argument(self, ctype, a):
        if ctype is ctypes.c_void_p:
            return None if a is None else self.where(a) if type(a) is int else {"!": type(a).__name__}
        if not isinstance(ctype, type(ctypes.c_int)):
            return "out"                                    # a result slot (void**)
        return a if type(a) in (int, float, bool) else {"!": type(a).__name__, "value": repr(a)}

    def call(self, name, args):
        real = getattr(self.real, name)
        assert len(args) == len(real.argtypes), "%s: %d arguments for %d" % (name, len(args), len(real.argtypes))
        event = [name, [self.argument(t, a) for t, a in zip(real.argtypes, args)]]
        self.events.append(event)
        if name.endswith("_bytes"):
            event.append(int(real(*args)))
            return event[2]
        if name in ("cimrgp_solve_queue", "cimrgp_front_queue"):
            args[1]._obj.value = self.queue_out
        return 0

    def result(self, v):
        if isinstance(v, torch.Tensor):
            return [self.where(v.data_ptr()), list(v.shape), list(v.stride())]
        if isinstance(v, (tuple, list)):
            return [self.result(e) for e in v]
        if isinstance(v, Stream):
            return ["stream", v.name, v.cuda_stream, v.device]
        if isinstance(v, dev.BlockMoments):
            return ["BlockMoments", list(v.proj.shape), len(v.colsum), len(v.colsum2), len(v.resid_sum), v.n]
        assert v is None or type(v) is int, v
        return v


_current = None                 # the recorder of the running case


class _Library(object):
    def __getattr__(self, name):
        if not name.startswith("cimrgp_"):
            raise AttributeError(name)
        return lambda *args: _current.call(name, args)


class _Cuda(object):
    @staticmethod
    def current_stream():
        return Stream("current", STREAM)

    @staticmethod
    def ExternalStream(handle, device=None):
        return Stream("external", handle, device)


class _Torch(object):
    cuda = _Cuda()

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        return _current.alloc("empty", torch.empty(*a, **k))

    @staticmethod
    def zeros(*a, **k):
        return _current.alloc("zeros", torch.zeros(*a, **k))

    @staticmethod
    def empty_like(*a, **k):
        return _current.alloc("empty", torch.empty_like(*a, **k))

    @staticmethod
    def as_tensor(*a, **k):
        return _current.alloc("as_tensor", torch.as_tensor(*a, **k), values=True)


@contextlib.contextmanager
def recording(rec):
    global _current
    _lib.load()
    saved = (_lib._lib, dev._stream, dev.torch, _current)
    _lib._lib, dev._stream, dev.torch, _current = _Library(), (lambda: STREAM), _Torch(), rec
    dev._LAYER_WORK.clear()
    try:
        yield rec
    finally:
        _lib._lib, dev._stream, dev.torch, _current = saved
        dev._LAYER_WORK.clear()


class Case(object):
    """The operands of one case; ``v`` is the variant (module docstring)."""

    def __init__(self, rec, v):
        self.rec, self.v = rec, v
        self.dtype = torch.float64 if v else torch.float32

    def t(self, name, *shape, **kw):
        """A tensor of the case's dtype (``dtype=`` another) called ``name``; variant 1: a view one row in and two
        columns in, into a buffer whose last dimension is padded.  ``view=False``: contiguous in both variants."""
        dtype = kw.pop("dtype", self.dtype)
        if not kw.pop("view", bool(self.v)):
            base = view = torch.zeros(shape, dtype=dtype)
        else:
            base = torch.zeros([s + 1 for s in shape[:-1]] + [dev.padded_ld(shape[-1] + 2)], dtype=dtype)
            view = base[tuple(slice(1, s + 1) for s in shape[:-1]) + (slice(2, shape[-1] + 2),)]
        self.rec.named.append((name, base))
        return view

    def mat(self, name, rows, cols, batch=None):
        """A padded (rows x ld) buffer as device.alloc_matrix makes it (``batch``: an arena of them); variant 1: a view."""
        shape = (rows, dev.padded_ld(cols)) if batch is None else (batch, rows, dev.padded_ld(cols))
        if not self.v:
            return self.t(name, *shape)
        base = torch.zeros([s + 1 for s in shape[:-1]] + [shape[-1] + 16], dtype=self.dtype)
        self.rec.named.append((name, base))
        return base[tuple(slice(1, s + 1) for s in shape[:-1]) + (slice(16, shape[-1] + 16),)]

    def opt(self, name, *shape, **kw):
        """An optional tensor: omitted in variant 0, given in variant 1."""
        return self.t(name, *shape, **kw) if self.v else None

    def n(self, value):
        """A size: a Python int in variant 0, a NumPy integer in variant 1."""
        return np.int64(value) if self.v else int(value)

    def x(self, value):
        """A real parameter: a Python float in variant 0, a NumPy float32 in variant 1."""
        return np.float32(value) if self.v else float(value)

    def ws(self, name, nbytes=4096, batch=None):
        return self.t(name, *((nbytes,) if batch is None else (batch, nbytes)), dtype=torch.uint8)

    def info(self, name="info", count=1):
        return self.t(name, count, dtype=torch.int32)

    def i64(self, name, count):
        return self.t(name, count, dtype=torch.int64)

    def stream(self, name, handle):
        self.rec.streams[handle] = name
        return Stream(name, handle)

    @property
    def flag(self):
        return bool(self.v)

    @property
    def cov(self):
        return _lib.COV_MATERN32 if self.v else _lib.COV_RBF


CASES = []                      # (name, function, refused)


def case(fn):
    CASES.append((fn.__name__, fn, False))
    return fn


def refused(fn):
    """A case that device.py refuses in Python: nothing may be allocated or called before the exception."""
    CASES.append((fn.__name__, fn, True))
    return fn


N, NS, M, D, Q, B = 40, 7, 5, 3, 2, 3            # points, test points, inducing points / carried rows, dims, outputs, blocks


# ---- Gram matrices, factorisation, solves ------------------------------------------------------------------------
@case
def rbf_gram(c):
    x = c.t("x", N, D)
    return dev.rbf_gram(x, c.x(0.7), 1.3, 0.01, lower_only=c.flag, out=None if not c.v else c.mat("k", N, N), cov=c.cov)


@case
def rbf_cross(c):
    xa, xb = c.t("xa", NS, D), c.t("xb", N, D)
    return dev.rbf_cross(xa, xb, 0.7, c.x(1.5), out=None if not c.v else c.mat("kab", NS, N), cov=c.cov)


@case
def potrf_workspace(c):
    return [dev.potrf_workspace_bytes(c.n(N), c.dtype), dev.potrf_workspace(c.n(300), c.dtype, "cpu")]


@case
def potrf(c):
    k = c.mat("k", N, N)
    return dev.potrf(k, c.n(N), ws=c.opt("ws", 1 << 16, dtype=torch.uint8), info=c.opt("info", 1, dtype=torch.int32))


@case
def potrf_rows(c):
    k, b = c.mat("k", N, N), c.mat("b", M, N)
    return dev.potrf_rows(k, c.n(N), b, c.n(M), ws=c.opt("ws", 1 << 16, dtype=torch.uint8),
                          info=c.opt("info", 1, dtype=torch.int32))


def _block_posterior(c, streams, with_xs=True):
    x, y = c.t("x", N, D), c.t("y", N, Q)
    xs = c.t("xs", NS, D) if with_xs else None
    kbuf, wbuf = c.mat("k", N, N), c.mat("w", NS + Q, N)
    alpha, z, mean, var = c.t("alpha", N, Q), c.t("z", N, Q), c.t("mean", NS, Q), c.t("var", NS)
    return dev.block_posterior(x, y, xs, c.x(0.7), 1.3, c.x(0.05), kbuf, wbuf, c.ws("ws"), c.info(), alpha, z, mean, var,
                               add_noise=c.flag, accumulate=not c.flag, scratch=c.opt("scratch", 2 * Q * N + 3),
                               streams=streams)


@case
def block_posterior(c):
    return _block_posterior(c, None)


@case
def block_posterior_staged(c):
    return _block_posterior(c, (c.stream("front", 0x5EED10), c.stream("factor", 0x5EED20), c.stream("solve", 0x5EED30)),
                            with_xs=bool(c.v))


@refused
def block_posterior_scratch_too_small(c):
    c.opt = lambda name, *shape, **kw: c.t(name, 2 * Q * N - 1)
    return _block_posterior(c, None)


@refused
def block_posterior_scratch_of_another_dtype(c):
    c.opt = lambda name, *shape, **kw: c.t(name, 2 * Q * N, dtype=torch.float64 if not c.v else torch.float32)
    return _block_posterior(c, None)


@case
def context_queues(c):
    given = c.stream("given", 0x5EED40)
    c.rec.queue_out = 0x5EED40 if c.v else 0x5EED50      # the stream itself (it owns no context) / another queue
    out = [dev.solve_queue(given), dev.front_queue(given)]
    c.rec.queue_out = STREAM if c.v else 0x5EED60
    return out + [dev.solve_queue(), dev.front_queue()]


@case
def potrf_rows_batched(c):
    k, ws, info = c.mat("k", N, N, batch=B), c.ws("ws", batch=B), c.info(count=B)
    if not c.v:
        return dev.potrf_rows_batched(k, N, k.stride(1), ws, info)
    b = c.mat("b", M, N, batch=B)
    return dev.potrf_rows_batched(k, c.n(N), c.n(k.stride(1)), ws, info, barena=b, m=c.n(M), ldb=c.n(b.stride(1)))


@case
def solve_lt_batched(c):
    k = c.mat("k", N, N, batch=B)
    return dev.solve_lt_batched(k, c.n(N), c.n(k.stride(1)), c.ws("ws", batch=B), c.t("z", B, N, Q, view=False))


@case
def solve_lt(c):
    return dev.solve_lt(c.mat("l", N, N), c.n(N), c.ws("ws"), c.t("z", N, Q))


@case
def potrs(c):
    return dev.potrs(c.mat("l", N, N), c.n(N), c.ws("ws"), c.t("rhs", N, Q), want_z=c.flag)


@case
def trsm_rows(c):
    return dev.trsm_rows(c.mat("l", N, N), c.n(N), c.ws("ws"), c.mat("b", M, N), c.n(M))


@case
def trsm_rows_lt(c):
    return dev.trsm_rows_lt(c.mat("l", N, N), c.n(N), c.ws("ws"), c.mat("b", M, N), c.n(M))


@case
def trsm_rows_lt_batched(c):
    return dev.trsm_rows_lt_batched(c.mat("l", N, N, batch=B), c.n(N), c.ws("ws", batch=B), c.mat("b", M, N, batch=B), c.n(M))


# ---- the layer calls ---------------------------------------------------------------------------------------------
def _layer_fit(c, n, tag=""):
    total = B * n
    x, y, train_out = c.t("x" + tag, total, D), c.t("y" + tag, total, Q), c.t("train_out" + tag, total, Q)
    k = c.mat("k" + tag, n, n, batch=B)
    return dev.layer_fit(x, y, c.opt("fbar" + tag, total, Q), train_out, c.i64("starts" + tag, B), c.n(n), c.x(0.7), 1.3,
                         -1.0 if not c.v else 0.02, c.x(0.01), 1e-6, c.opt("shared_bias" + tag, Q), c.opt("shared_noise" + tag, 1),
                         k, c.ws("ws" + tag, batch=B), c.info("info" + tag, B), c.t("bias" + tag, B, Q), c.t("noise" + tag, B),
                         c.t("z" + tag, B, n, Q), c.t("alpha" + tag, B, n, Q), cov=c.cov)


@case
def layer_fit(c):
    """Twice at one shape (the work areas are allocated once), then at another (they are replaced)."""
    return [_layer_fit(c, N), _layer_fit(c, N, "'"), _layer_fit(c, N + 9, "''")]


def _layer_args(c):
    x, xs = c.t("x", B * N, D), c.t("xs", B * NS, D)
    return (x, c.i64("starts", B), c.n(N), xs, c.i64("t_starts", B), c.n(NS), c.x(0.7), 1.3, c.mat("l", N, N, batch=B),
            c.ws("ws", batch=B))


@case
def layer_predict(c):
    return dev.layer_predict(*_layer_args(c), c.t("z", B, N, Q), c.opt("bias", B, Q), c.opt("noise", B), c.t("mean", B * NS, Q),
                             c.opt("var", B * NS), cov=c.cov)


@case
def layer_joint_cov(c):
    return dev.layer_joint_cov(*_layer_args(c), c.opt("diag", B), c.mat("c", NS, NS, batch=B),
                               cws_arena=None if not c.v else c.ws("cws", batch=B),
                               info=c.opt("info", B, dtype=torch.int32), cov=c.cov)


@case
def layer_predict_grad(c):
    return dev.layer_predict_grad(*_layer_args(c), c.t("alpha", B, N, Q, view=False), c.t("mean_grad", B * NS, D, Q, view=False),
                                  c.opt("var_grad", B * NS, D), cov=c.cov)


@case
def normal_fill(c):
    seed = 12345 if not c.v else -3          # a negative seed wraps to 64 bits
    return dev.normal_fill(seed, c.i64("keys", B), c.n(1), c.n(4), c.n(NS), c.t("z", B, 4, 16))


@case
def layer_sample(c):
    return dev.layer_sample(c.mat("l", NS, NS, batch=B), c.n(NS), c.t("z", B, 4, 16), c.n(4), c.i64("t_starts", B),
                            c.t("out", 4, B * NS))


def _layer_lml_args(c):
    total = B * N
    return (c.t("x", total, D), c.t("y", total, Q), c.opt("fbar", total, Q), c.i64("starts", B), c.n(N))


@case
def layer_lml_grad(c):
    k = c.mat("k", N, N, batch=B)
    return [dev.layer_lml_scratch_bytes(c.n(N), c.n(Q), c.n(B), c.dtype),
            dev.layer_lml_grad(*_layer_lml_args(c), c.x(0.7), 1.3, c.x(0.05), c.opt("shared_bias", Q), k, c.mat("kinv", N, N, batch=B),
                               c.ws("ws", batch=B), c.info(count=B), c.t("out", B, 4, dtype=torch.float64), cov=c.cov)]


@case
def layer_lml_grad_ard(c):
    k = c.mat("k", N, N, batch=B)
    return [dev.layer_lml_ard_scratch_bytes(c.n(N), c.n(Q), c.n(B), c.dtype),
            dev.layer_lml_grad_ard(*_layer_lml_args(c), 1.3, c.x(0.05), c.opt("shared_bias", Q), k, c.mat("kinv", N, N, batch=B),
                                   c.ws("ws", batch=B), c.info(count=B), c.t("out", B, D + 3, dtype=torch.float64), cov=c.cov)]


# ---- one block: prediction, gradients, leave-one-out, likelihood -------------------------------------------------
@case
def predict_mean(c):
    x, alpha, xs = c.t("x", N, D), c.t("alpha", N, Q), c.t("xs", NS, D)
    return dev.predict_mean(x, alpha, xs, c.x(0.7), 1.3, bias=c.opt("bias", Q), out=c.opt("out", NS, Q), accumulate=True,
                            cov=c.cov)


@case
def predict_from_w(c):
    w = c.mat("w", NS, N)
    return dev.predict_from_w(w, c.n(NS), c.n(N), c.opt("z", N, Q), c.x(1.3), extra_var=c.x(0.1), bias=c.opt("bias", Q),
                              mean_out=c.opt("mean", NS, Q), var_out=c.t("var", NS), accumulate=c.flag,
                              extra_var_dev=c.opt("noise", 1))


@case
def cov_predict_grad(c):
    x, xs = c.t("x", N, D), c.t("xs", NS, D)
    beta = c.mat("beta", NS, N)
    return [dev.cov_predict_grad(x, c.t("alpha", N, Q), xs, c.x(0.7), 1.3, beta=beta if c.v else None,
                                 mean_grad=c.t("mean_grad", NS, D, Q, view=False),
                                 var_grad=c.opt("var_grad", NS, D), accumulate=c.flag, cov=c.cov),
            dev.cov_predict_grad(x, None, xs, 0.7, 1.3, beta=beta, mean_grad=c.t("mg", NS, D, Q + 1, view=False) if c.v else None,
                                 var_grad=c.t("vg", NS, D, view=False), cov=c.cov)]


@case
def trtri_rows(c):
    return dev.trtri_rows(c.mat("l", N, N), c.n(N), c.ws("ws"), c.n(8), c.n(M), out=None if not c.v else c.mat("u", M, N))


@case
def kinv_diag(c):
    return [dev.kinv_diag_scratch_bytes(c.n(N), c.n(16), c.dtype),
            dev.kinv_diag(c.mat("l", N, N), c.n(N), c.ws("ws"), c.n(0 if not c.v else 1 << 30), out=c.opt("out", N)),
            dev.kinv_diag(c.mat("l2", 300, 300), c.n(300), c.ws("ws2"), 300000)]


@case
def kinv_diag_batched(c):
    return [dev.kinv_diag_batched(c.mat("l", N, N, batch=B), c.n(N), c.ws("ws", batch=B), c.n(0 if not c.v else 1 << 30),
                                  out=c.opt("out", B, N)),
            dev.kinv_diag_batched(c.mat("l2", 300, 300, batch=B), c.n(300), c.ws("ws2", batch=B), 800000)]


@case
def loo(c):
    return [dev.loo(c.t("y", N, Q), c.t("alpha", N, Q), c.t("diag", N), mean_out=c.opt("mean", N, Q), var_out=c.t("var", N)),
            dev.loo(c.t("yb", B * N, Q), c.t("alphab", B, N, Q, view=False), c.t("diagb", B, N, view=False),
                    mean_out=c.t("meanb", B * N, Q), var_out=c.opt("varb", B * N), starts=c.i64("starts", B))]


@case
def block_stats(c):
    return dev.block_stats(c.t("y", N, Q), c.opt("fbar", N, Q), stats_out=c.opt("stats", Q + 1))


@case
def residual(c):
    return dev.residual(c.t("y", N, Q), c.opt("fbar", N, Q), c.opt("bias", Q), out=c.opt("out", N, Q))


@case
def train_mean(c):
    return dev.train_mean(c.t("r", N, Q), c.t("alpha", N, Q), c.opt("bias", Q), c.t("noise", 1), c.t("out", N, Q),
                          accumulate=c.flag)


@case
def add_diag(c):
    return dev.add_diag(c.mat("k", N, N), c.n(N), c.t("noise", 1))


@case
def noise_from_stats(c):
    return dev.noise_from_stats(c.t("stats", Q + 1), c.n(Q), c.x(0.01), 1e-6, out=c.opt("out", 1))


@case
def logdet_half(c):
    return dev.logdet_half(c.mat("l", N, N), c.n(N))


@case
def syrk_lower(c):
    return dev.syrk_lower(c.mat("c", N, N), c.mat("a", N, M), c.n(N), c.n(M))


@case
def lml_grad(c):
    return dev.lml_grad(c.t("x", N, D), c.mat("kinv", N, N), c.n(N), c.t("alpha", N, Q), c.x(0.7), 1.3, c.x(0.05), cov=c.cov)


@case
def lml_grad_ard(c):
    return dev.lml_grad_ard(c.t("x", N, D), c.mat("kinv", N, N), c.n(N), c.t("alpha", N, Q), c.x(1.3), 0.05, cov=c.cov)


# ---- sparse (inducing-point) blocks ------------------------------------------------------------------------------
@case
def wsyrk_tn(c):
    a = c.mat("a", N, M)
    return [dev.wsyrk_tn_scratch_bytes(c.n(N), c.n(M), c.n(Q), c.dtype),
            dev.wsyrk_tn(a, c.n(N), c.n(M), c.t("w", N), r=c.opt("r", N, Q), diag_add=c.x(1.0),
                         out=None if not c.v else c.mat("out", M, M), g=c.opt("g", M, Q),
                         scratch=None if not c.v else c.ws("scratch", 1 << 16)),
            dev.wsyrk_tn(a, N, M, c.t("w2", N), r=c.t("r2", N, Q))]


def _lambda_outputs(c):
    return dict(lam=c.opt("lam", N), w=c.opt("w", N), sums=c.opt("sums", 3, dtype=torch.float64))


@case
def sparse_lambda(c):
    return dev.sparse_lambda(c.mat("a", N, M), c.n(N), c.n(M), c.x(1.3), 0.05, c.n(c.v), **_lambda_outputs(c))


@case
def sparse_lambda_dev(c):
    return dev.sparse_lambda_dev(c.mat("a", N, M), c.n(N), c.n(M), c.x(1.3), c.t("noise", 1), c.n(c.v), **_lambda_outputs(c))


@refused
def sparse_lambda_dev_noise_of_another_dtype(c):
    return dev.sparse_lambda_dev(c.mat("a", N, M), N, M, 1.3, c.t("noise", 1, dtype=torch.int32), 0)


@refused
def sparse_lambda_dev_noise_empty(c):
    return dev.sparse_lambda_dev(c.mat("a", N, M), N, M, 1.3, c.t("noise", 1)[:0], 0)


def _tail_args(c, same_pitch=True):
    astar = c.mat("astar", NS, M) if c.v or not same_pitch else None
    wstar = c.mat("wstar", NS, M if same_pitch else M + 16)
    return astar, wstar, c.n(NS), c.n(M), c.opt("gamma", M, Q), c.x(1.3)


@case
def sparse_tail(c):
    return dev.sparse_tail(*_tail_args(c), extra_var=c.x(0.05), mean_out=c.opt("mean", NS, Q), var_out=c.t("var", NS),
                           accumulate=c.flag)


@refused
def sparse_tail_pitch_mismatch(c):
    return dev.sparse_tail(*_tail_args(c, same_pitch=False), var_out=c.t("var", NS))


@case
def sparse_tail_dev(c):
    return dev.sparse_tail_dev(*_tail_args(c), extra_var=c.x(0.05), bias=c.opt("bias", Q), extra_var_dev=c.opt("noise", 1),
                               mean_out=c.opt("mean", NS, Q), var_out=c.t("var", NS), accumulate=c.flag)


@refused
def sparse_tail_dev_pitch_mismatch(c):
    return dev.sparse_tail_dev(*_tail_args(c, same_pitch=False), var_out=c.t("var", NS))


@refused
def sparse_tail_dev_bias_refused(c):
    """Variant 0: too short; variant 1: another dtype."""
    astar, wstar = c.mat("astar", NS, M), c.mat("wstar", NS, M)
    bias = c.t("bias", Q, dtype=torch.float32) if c.v else c.t("bias", Q - 1)
    return dev.sparse_tail_dev(astar, wstar, NS, M, c.t("gamma", M, Q), 1.3, bias=bias, mean_out=c.t("mean", NS, Q))


@refused
def sparse_tail_dev_extra_var_refused(c):
    """Variant 0: empty; variant 1: another dtype."""
    astar, wstar = c.mat("astar", NS, M), c.mat("wstar", NS, M)
    extra = c.t("noise", 1, dtype=torch.float32) if c.v else c.t("noise", 1)[:0]
    return dev.sparse_tail_dev(astar, wstar, NS, M, None, 1.3, extra_var_dev=extra, var_out=c.t("var", NS))


def _pair_grad(c, fn, nsums):
    xa, xb, g = c.t("xa", N, D), c.t("xb", M, D), c.mat("g", N, M)
    full = fn(xa, xb, g, c.x(0.7), 1.3, scale=c.x(2.0), accumulate=c.flag, sums=c.opt("sums", nsums, dtype=torch.float64),
              db=c.opt("db", M, D), cov=c.cov, scratch=None if not c.v else c.ws("scratch", 1 << 16))
    # an output that is not wanted is neither allocated nor passed, given or not
    return [full, fn(xa, xb, g, 0.7, 1.3, want_sums=bool(c.v), want_db=not c.v, sums=c.opt("sums2", nsums, dtype=torch.float64),
                     db=c.opt("db2", M, D))]


@case
def cov_pair_grad(c):
    return [dev.cov_pair_grad_scratch_bytes(c.n(N), c.n(M), c.n(D))] + _pair_grad(c, dev.cov_pair_grad, 2)


@case
def cov_pair_grad_ard(c):
    return [dev.cov_pair_grad_ard_scratch_bytes(c.n(N), c.n(M), c.n(D))] + _pair_grad(c, dev.cov_pair_grad_ard, 1 + D)


@case
def sparse_grad_rows(c):
    return dev.sparse_grad_rows(c.mat("v", N, M), c.n(N), c.n(M), c.t("gamma", M, Q), c.t("r", N, Q), c.t("w", N), c.n(c.v),
                                c.x(0.05), beta=c.opt("beta", N, Q), t=c.opt("t", N), sums=c.opt("sums", 2, dtype=torch.float64))


@case
def sparse_grad_combine(c):
    return dev.sparse_grad_combine(c.mat("a", N, M), c.mat("y", N, M), c.n(N), c.n(M), c.t("beta", N, Q), c.t("b", M, Q),
                                   c.t("w", N), c.t("t", N))


@case
def cov_cross_grad(c):
    return dev.cov_cross_grad(c.t("xa", NS, D), c.t("xb", M, D), c.x(0.7), 1.3, c.mat("out", NS + c.v, M, batch=D + 1), cov=c.cov)


@refused
def cov_cross_grad_out_refused(c):
    """Variant 0: too few slabs; variant 1: too few rows."""
    out = c.mat("out", NS - 1, M, batch=D + 1) if c.v else c.mat("out", NS, M, batch=D)
    return dev.cov_cross_grad(c.t("xa", NS, D), c.t("xb", M, D), 0.7, 1.3, out)


@refused
def cov_cross_grad_out_not_slabs(c):
    """Variant 0: a matrix; variant 1: columns not contiguous."""
    out = c.t("out", D + 1, NS, M, 2)[..., 0] if c.v else c.mat("out", NS, M)
    return dev.cov_cross_grad(c.t("xa", NS, D), c.t("xb", M, D), 0.7, 1.3, out)


@case
def sparse_tail_grad(c):
    w = c.mat("wslabs", NS, M, batch=D + 1)
    return dev.sparse_tail_grad(c.mat("aslabs", NS, M, batch=D + 1) if c.v else None, w, c.n(NS), c.n(M), c.opt("gamma", M, Q),
                                mean_grad=c.opt("mean_grad", NS, D, Q), var_grad=c.t("var_grad", NS, D), accumulate=c.flag)


@refused
def sparse_tail_grad_layout_mismatch(c):
    """Variant 0: another row pitch; variant 1: another slab stride."""
    a = c.mat("aslabs", NS + 1, M, batch=D + 1)[:, :NS] if c.v else c.mat("aslabs", NS, M + 16, batch=D + 1)
    return dev.sparse_tail_grad(a, c.mat("wslabs", NS, M, batch=D + 1), NS, M, None, var_grad=c.t("var_grad", NS, D))


@case
def sparse_loo(c):
    return dev.sparse_loo(c.mat("a", N, M), c.mat("v", N, M), c.n(N), c.n(M), c.t("gamma", M, Q), c.t("r", N, Q), c.x(1.3), 0.05,
                          c.n(c.v), c.info("bad"), mean_out=c.opt("mean", N, Q), var_out=c.opt("var", N))


@refused
def sparse_loo_pitch_mismatch(c):
    return dev.sparse_loo(c.mat("a", N, M), c.mat("v", N, M + 16), N, M, c.t("gamma", M, Q), c.t("r", N, Q), 1.3, 0.05, 0,
                          c.info("bad"))


@refused
def sparse_loo_bad_refused(c):
    """Variant 0: empty; variant 1: another dtype."""
    bad = c.i64("bad", 1) if c.v else c.info("bad")[:0]
    return dev.sparse_loo(c.mat("a", N, M), c.mat("v", N, M), N, M, c.t("gamma", M, Q), c.t("r", N, Q), 1.3, 0.05, 0, bad)


@case
def sparse_joint_cov(c):
    return dev.sparse_joint_cov(c.t("xs", NS, D), c.x(0.7), 1.3, c.x(0.05), c.mat("astar", NS, M), c.mat("wstar", NS, M), c.n(M),
                                c.mat("c", NS, NS), cws=None if not c.v else c.ws("cws", 777),
                                info=c.opt("info", 1, dtype=torch.int32), cov=c.cov)


@refused
def sparse_joint_cov_pitch_mismatch(c):
    return dev.sparse_joint_cov(c.t("xs", NS, D), 0.7, 1.3, 0.05, c.mat("astar", NS, M), c.mat("wstar", NS, M + 16), M,
                                c.mat("c", NS, NS))


# ---- reduced-rank (Laplacian basis) blocks -----------------------------------------------------------------------
INTERVAL = [[1.5], [2.0], [2.5]]
EAU = np.arange(Q * M, dtype=np.float32).reshape(Q, M) / 4


@case
def laplace_basis(c):
    return dev.laplace_basis(c.t("x", N, D, view=False), INTERVAL, c.n(M), out=c.opt("phi", N, M, view=False))


@case
def laplace_basis_interval_of_another_dimension(c):
    return dev.laplace_basis(c.t("x", N, D, view=False), INTERVAL[:2], M, out=c.t("phi", N, M, view=False))


@case
def basis_moments(c):
    return dev.basis_moments(c.t("x", N, D, view=False), np.asarray(INTERVAL), c.n(M), c.t("y", N, Q, view=False),
                             c.opt("fbar", N, Q, view=False), c.opt("fvar", N, view=False), EAU if c.v else EAU.tolist())


@case
def basis_apply(c):
    return dev.basis_apply(c.t("x", N, D, view=False), INTERVAL, c.n(M), EAU, bias=[0.5, 1.5] if c.v else None,
                           c2=np.ones(M) if c.v else None, bias_var=c.x(0.25), mean=c.opt("mean", N, Q, view=False),
                           var=c.t("var", N, view=False), accumulate=c.flag)


@case
def basis_operands_not_contiguous(c):
    """Variant 0: basis_moments; variant 1: basis_apply.  The host arrays are on the device by then."""
    x = c.t("x", N, D, view=True)
    if c.v:
        return dev.basis_apply(x, INTERVAL, M, EAU, mean=c.t("mean", N, Q))
    return dev.basis_moments(x, INTERVAL, M, c.t("y", N, Q), None, None, EAU)


# ---- refusals shared by many wrappers ----------------------------------------------------------------------------
def _unknown_cov_calls(c):
    x, xs, k, ws = c.t("x", N, D), c.t("xs", NS, D), c.mat("k", N, N, batch=B), c.ws("ws", batch=B)
    layer = (x, c.i64("starts", B), N, xs, c.i64("t_starts", B), NS, 0.7, 1.3, k, ws)
    g, y, out = c.mat("g", N, NS), c.t("y", N, Q), c.t("out", B, 4, dtype=torch.float64)
    return [
        lambda cov: dev.rbf_gram(x, 0.7, 1.3, cov=cov),
        lambda cov: dev.rbf_cross(xs, x, 0.7, 1.3, cov=cov),
        lambda cov: dev.layer_fit(x, y, None, y, layer[1], N, 0.7, 1.3, -1.0, 0.01, 1e-6, None, None, k, ws, c.info(count=B), y, y, y, y,
                                  cov=cov),
        lambda cov: dev.layer_predict(*layer, y, None, None, y, None, cov=cov),
        lambda cov: dev.layer_joint_cov(*layer, None, k, cov=cov),
        lambda cov: dev.cov_predict_grad(x, y, xs, 0.7, 1.3, mean_grad=y, cov=cov),
        lambda cov: dev.layer_predict_grad(*layer, y, y, y, cov=cov),
        lambda cov: dev.cov_pair_grad(x, xs, g, 0.7, 1.3, cov=cov),
        lambda cov: dev.cov_pair_grad_ard(x, xs, g, 0.7, 1.3, cov=cov),
        lambda cov: dev.cov_cross_grad(xs, x, 0.7, 1.3, k, cov=cov),
        lambda cov: dev.sparse_joint_cov(xs, 0.7, 1.3, 0.05, g, g, NS, g, cov=cov),
        lambda cov: dev.layer_lml_grad(x, y, None, layer[1], N, 0.7, 1.3, 0.05, None, k, k, ws, c.info("i2", B), out, cov=cov),
        lambda cov: dev.layer_lml_grad_ard(x, y, None, layer[1], N, 1.3, 0.05, None, k, k, ws, c.info("i3", B), out, cov=cov),
        lambda cov: dev.predict_mean(x, y, xs, 0.7, 1.3, cov=cov),
        lambda cov: dev.lml_grad(x, g, N, y, 0.7, 1.3, 0.05, cov=cov),
        lambda cov: dev.lml_grad_ard(x, g, N, y, 1.3, 0.05, cov=cov),
    ]


@refused
def unknown_covariance(c):
    """Every wrapper with a ``cov`` argument, with an id past the last (variant 0) and a negative one (variant 1)."""
    messages = []
    for call in _unknown_cov_calls(c):
        try:
            call(-1 if c.v else 4)
            messages.append(None)
        except ValueError as e:
            messages.append(str(e))
    assert None not in messages
    raise ValueError(" | ".join(sorted(set(messages))))


@case
def unsupported_dtype(c):
    """KeyError from the dtype table: at the call, after the output was allocated (variant 0), and in a size query."""
    try:
        if c.v:
            dev.potrf_workspace_bytes(N, torch.float16)
        else:
            dev.rbf_gram(c.t("x", N, D, dtype=torch.float16), 0.7, 1.3)
    except KeyError as e:
        return [len(c.rec.events), 1 if e.args == (torch.float16,) else 0]


def run_case(fn, v):
    """One case, one variant: {"events": [...], "returns": ... | "raises": [type, message], "layer_work": [...]}."""
    with recording(Recorder()) as rec:
        out = {}
        try:
            out["returns"] = rec.result(fn(Case(rec, v)))
        except AssertionError:
            raise
        except Exception as e:          # a Python-side refusal of device.py
            out["raises"] = [type(e).__name__, str(e)]
        out["events"] = rec.events
        if dev._LAYER_WORK:
            out["layer_work"] = [[[k[0], str(k[1]), k[2]], list(hit[0])] for k, hit in dev._LAYER_WORK.items()]
        return out


def run_all():
    return {"%s[%d]" % (name, v): run_case(fn, v) for name, fn, _ in CASES for v in (0, 1)}


def dumps(entry):
    """The JSON text the comparison is made on: it keeps 1, 1.0 and true apart, which == on the loaded values does not."""
    return json.dumps(entry, sort_keys=True)


if __name__ == "__main__":
    log = run_all()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), dumps(v)) for k, v in log.items()) + "\n}\n")
    print("%d cases, %d C calls -> %s" % (len(log), sum(1 for e in log.values() for ev in e["events"] if ev[0] != "alloc"), GOLDEN))
