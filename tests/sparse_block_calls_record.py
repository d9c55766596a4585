"""Every C call and every host read-back of ``Sparse.SparseBlock``, recorded on the CPU with the stand-in library of
tests/device_calls_record.py: shared by tests/test_sparse_block_calls_host.py, which replays the cases below against the
working tree's Sparse.py and compares with tests/golden/sparse_block_calls.json.  Run as a script
(``python tests/sparse_block_calls_record.py``) it writes that file; the committed one was written ONCE, from the commit
before the block's covariance became one object (``Sparse.BlockCovariance``), with that commit's package on the path, and
pins what the block asks of C, in which order, across such rewrites.

The operands are CPU tensors of zeros and every C function is the stand-in, so the numbers mean nothing: what is recorded
is the sequence.  An event is

    ["op", name]                   an operation of the case begins
    [C function, [argument, ...]]  a call; a scalar as itself (the JSON text keeps int, float and bool apart), null as null,
                                   a pointer as "<tensor>+<byte offset>"
    ["read", how, shape, dtype]    ``.cpu()`` or ``.item()`` of a tensor
    ["raises", type, message]      the exception that ended an operation

A pointer's tensor is the case's name for an operand (``x``, ``z``, ``r``, ``xs``, ``mean`` ..), or ``t<k>`` for a tensor the
block made itself: k counts such tensors by their first appearance in a call, whoever allocated them and when, so the log
does not depend on the order of allocations.  Every tensor that reached a call is kept alive to the end of the case: no
address is met twice.  What ``empty`` / ``empty_like`` return inside ``device`` is zero-filled, or the count of
non-positive lambda would be read from uninitialised memory and trip the block's failure check.

Every case runs in the recorder's two variants, here float32 and float64 alone (the operands are contiguous in both: the
block takes them as the plugins pass them).  Shapes: n = 40, m = 6, d = 2, q = 2; ns = 300 test rows with
``budget_bytes=1``, so that the chunked operations make two chunks, of 256 and 44 rows.

Every operation of the block runs under the stand-in; none is left to tools/sparse_ab.py for that reason.  What the
stand-in cannot show is the arithmetic: tools/sparse_ab.py compares that, bit for bit, on the GPU."""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import device_calls_record as base  # noqa: E402
from cimrgp_amd import device as dev, device_linear as devl  # noqa: E402
from cimrgp_amd.KernelClass import DenseMaternKernel, RBFKernel  # noqa: E402
from cimrgp_amd.Sparse import SparseBlock  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_block_calls.json")
N, M, D, Q, NS = 40, 6, 2, 2, 300
ELLS, LINEAR = (0.7, 1.3), (0.5, 0.2)
SF, NOISE, JITTER = 1.3, 0.05, 1e-6


class Recorder(base.Recorder):
    """The base recorder with pointers named by first appearance and no allocation events."""

    def __init__(self):
        base.Recorder.__init__(self)
        self.known = []             # (label, storage address, bytes, the storage's tensor), in order of first appearance
        self.made = 0

    def alloc(self, kind, t, values=False):
        if kind == "empty":
            t.zero_()
        self.allocs.append(t)
        return t

    def meet(self, t):
        """Name the storage of a tensor that reaches a call, and keep it."""
        start = t.untyped_storage().data_ptr()
        if any(s == start for _, s, _, _ in self.known):
            return
        for label, operand in self.named:
            if operand.untyped_storage().data_ptr() == start:
                break
        else:
            label, self.made = "t%d" % self.made, self.made + 1
        self.known.append((label, start, max(t.untyped_storage().nbytes(), 1), t))

    def where(self, address):
        if address in self.streams:
            return self.streams[address]
        for label, start, nbytes, _ in self.known:
            if start <= address < start + nbytes:
                return "%s+%d" % (label, address - start)
        raise AssertionError("pointer %#x belongs to no tensor that reached a call" % address)


@contextlib.contextmanager
def recording(rec):
    """base.recording, and: every tensor argument of ``device._call`` is met by the recorder before the call is
    marshalled; ``Tensor.cpu`` and ``Tensor.item`` leave a read event."""
    real_call, real_cpu, real_item = dev._call, torch.Tensor.cpu, torch.Tensor.item

    def call(name, *args, **kw):
        for a in args:
            if isinstance(a, torch.Tensor):
                rec.meet(a)
        return real_call(name, *args, **kw)

    def read(how, real):
        def method(self, *a, **k):
            rec.events.append(["read", how, list(self.shape), str(self.dtype)])
            return real(self, *a, **k)
        return method

    with base.recording(rec):
        dev._call = devl._call = call
        torch.Tensor.cpu, torch.Tensor.item = read("cpu", real_cpu), read("item", real_item)
        try:
            yield rec
        finally:
            dev._call = devl._call = real_call
            torch.Tensor.cpu, torch.Tensor.item = real_cpu, real_item


class Case(base.Case):
    """Named operands (contiguous in both variants) and the operations of a block, each under its own ``op`` event."""

    def t(self, name, *shape, **kw):
        kw["view"] = False
        return base.Case.t(self, name, *shape, **kw)

    def block(self, arm="plain", approximation="fitc", kernel=None, **kw):
        if kernel is None:
            kernel = RBFKernel(l=1.0 if "ard" in arm else 0.7, sf=SF, noise=NOISE)
        if "ard" in arm:
            kw["lengthscales"] = ELLS
        if "linear" in arm:
            kw["linear"] = LINEAR
        return SparseBlock(self.t("x", N, D), self.t("z", M, D), kernel, approximation, JITTER, **kw)

    def op(self, name, fn):
        self.rec.events.append(["op", name])
        try:
            fn()
        except AssertionError:
            raise
        except Exception as e:
            self.rec.events.append(["raises", type(e).__name__, str(e)])

    def plugin_operations(self, blk, queries):
        r, xs = self.t("r", N, Q), self.t("xs", NS, D)
        mean, var = self.t("mean", NS, Q), self.t("var", NS)
        self.op("fit", lambda: blk.fit(r))
        self.op("log_marginal_likelihood", blk.log_marginal_likelihood)
        self.op("predict", lambda: blk.predict(xs, mean, var, budget_bytes=1))
        self.op("predict_mean_only", lambda: blk.predict(xs, mean, None, budget_bytes=1))
        self.op("predict_var_only", lambda: blk.predict(xs, None, var, budget_bytes=1))
        self.op("predict_include_noise", lambda: blk.predict(xs, mean, var, include_noise=True, budget_bytes=1))
        self.op("lml_grad", lambda: blk.lml_grad(r))
        self.op("lml_grad_theta_only", lambda: blk.lml_grad(r, want_z=False))
        if not queries:
            return
        mean_grad, var_grad = self.t("mean_grad", NS, D, Q), self.t("var_grad", NS, D)
        self.op("predict_grad", lambda: blk.predict_grad(xs, mean_grad, var_grad, budget_bytes=1))
        self.op("predict_grad_mean_only", lambda: blk.predict_grad(xs, mean_grad, None, budget_bytes=1))
        self.op("loo", lambda: blk.loo(r, self.t("loo_mean", N, Q), self.t("loo_var", N), budget_bytes=1))
        self.op("joint_cov", lambda: blk.joint(xs, cov_out=self.t("cov_out", NS, NS), include_noise=True))
        self.op("joint_samples", lambda: blk.joint(xs, samples=self.t("samples", 3, NS), seed=7))


CASES = []                      # (name, function)


def _plugin_case(arm, approximation, matern=False):
    def fn(c):
        kernel = DenseMaternKernel(nu=1.5, l=1.0 if "ard" in arm else 0.7, sf=SF, noise=NOISE) if matern else None
        c.plugin_operations(c.block(arm, approximation, kernel), queries="linear" not in arm)
    CASES.append(("%s_%s%s" % (arm, approximation, "_matern32" if matern else ""), fn))


for _arm in ("plain", "ard", "linear", "ard_linear"):
    for _approximation in ("fitc", "vfe"):
        _plugin_case(_arm, _approximation)
_plugin_case("ard", "vfe", matern=True)
_plugin_case("ard_linear", "fitc", matern=True)


def _layer_case(name, approximation, noise):
    def fn(c):
        blk = c.block("plain", approximation, RBFKernel(l=0.7, sf=SF, noise=noise), device_noise=True)
        y, f_bar, train_out = c.t("y", N, Q), c.t("f_bar", N, Q), c.t("train_out", N, Q)
        xs, mean, var = c.t("xs", NS, D), c.t("mean", NS, Q), c.t("var", NS)
        c.op("fit_layer", lambda: blk.fit_layer(y, f_bar, train_out))
        c.op("fit_layer_shared", lambda: blk.fit_layer(y, f_bar, train_out, c.t("shared_bias", Q), c.t("shared_noise", 1)))
        c.op("predict_layer", lambda: blk.predict_layer(xs, mean, var, add_noise=True, budget_bytes=1))
        c.op("predict_layer_mean_only", lambda: blk.predict_layer(xs, mean, budget_bytes=1))
        c.op("predict_grad_refused", lambda: blk.predict_grad(xs))
    CASES.append((name, fn))


_layer_case("layer_fitc_noise_from_the_targets", "fitc", None)
_layer_case("layer_vfe_noise_fixed", "vfe", NOISE)


def ready_for_refusals(c):
    """``_ready_for`` refuses before any C call: a block with a linear term, fitted or not, and a block not yet fitted."""
    r, xs = c.t("r", N, Q), c.t("xs", NS, D)
    for arm in ("ard_linear", "linear", "plain"):
        blk = c.block(arm, "vfe")
        if arm == "linear":
            blk.gamma = c.t("gamma", M, Q)          # as after a fit
        c.op("%s_predict_grad" % arm, lambda: blk.predict_grad(xs))
        c.op("%s_loo" % arm, lambda: blk.loo(r))
        c.op("%s_joint" % arm, lambda: blk.joint(xs))
    blk = c.block("plain")
    c.op("predict_before_fit", lambda: blk.predict(xs))
    c.op("predict_layer_before_fit", lambda: blk.predict_layer(xs, None))
    c.op("log_marginal_likelihood_before_fit", blk.log_marginal_likelihood)


CASES.append(("ready_for_refusals", ready_for_refusals))


def run_case(fn, v):
    with recording(Recorder()) as rec:
        fn(Case(rec, v))
        return {"events": rec.events}


def run_all():
    return {"%s[%d]" % (name, v): run_case(fn, v) for name, fn in CASES for v in (0, 1)}


def calls(entry):
    return [e for e in entry["events"] if e[0] not in ("op", "read", "raises")]


if __name__ == "__main__":
    log = run_all()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), base.dumps(v)) for k, v in log.items()) + "\n}\n")
    print("%d cases, %d C calls -> %s" % (len(log), sum(len(calls(e)) for e in log.values()), GOLDEN))
