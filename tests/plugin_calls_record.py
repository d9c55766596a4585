"""Every C call and every host read-back of the regression plugins (cimrgp_amd/RegressionInput.py), recorded on the CPU with
the stand-in library of tests/device_calls_record.py: shared by tests/test_plugin_calls_host.py, which replays the cases
below against the working tree and compares with tests/golden/plugin_calls.json.  Run as a script
(``python tests/plugin_calls_record.py``) it writes that file; the committed one was written ONCE, with the package of the
commit before the plugins got their common inducing-point base on the path, and pins what a plugin asks of C, in which
order and with which host reads in between, what it refuses and with which words, and the signature of every public
method, across such rewrites.

The events are those of tests/sparse_block_calls_record.py (``op``, a call, ``read``, ``raises``), and

    ["attr", name, shape(, values)]    an attribute a fit left: ``inducing_ids`` with its values, ``inducing_inputs`` and
                                       ``lengthscales`` by shape (null: the attribute is None)

A plugin takes NumPy arrays and uploads them itself, so every pointer is a ``t<k>``.  For the length of a case
``device.require_gpu`` returns the CPU device, and ``device_svgp._call`` / ``device_psi._call`` are the recording call
that sparse_block_calls_record.recording puts into ``device`` and ``device_linear``; all of it is undone on exit.

Shapes are the block log's: n = 40, m = 6, d = 2, q = 2, and 300 test rows with ``budget_bytes=1`` wherever a method takes
it, which makes two chunks of 256 and 44 rows.  Every case is float64 (two of the plugins have nothing else).  A plugin
case runs the five further queries before ``fit`` (a refusal, or "call fit() before"), ``fit`` with ``optimize=False``,
``predict``, ``predict_with_variance``, the five queries again and the objective calls the plugin has.  One case per plugin
class records the refusals of bad constructor arguments (those the host tests try) and of a fit, and the entry
``signatures`` holds ``str(inspect.signature(m))`` of every public method of every exported plugin class.

The optimiser cases (``optimize=True, max_iters=2``) are in the log because two recordings from that commit gave the same
text: under the stand-in every number the optimiser sees is zero or NaN and its path depends on SciPy alone.  The script
checks that again whenever it writes the file.  What the stand-in cannot show is the arithmetic: tools/sparse_ab.py
compares that, bit for bit, on the GPU."""
import contextlib
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import device_calls_record as base  # noqa: E402
import sparse_block_calls_record as blocks  # noqa: E402
import cimrgp_amd as ca  # noqa: E402
from cimrgp_amd import device as dev, device_psi as devp, device_svgp as devs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plugin_calls.json")
N, M, D, Q, NS = 40, 6, 2, 2, 300

_rng = np.random.RandomState(0)
X = _rng.uniform(-2.0, 2.0, size=(N, D))
Y = np.stack([np.sin(2.0 * X[:, 0] + c) + 0.4 * X[:, 1] for c in range(Q)], axis=1) + 0.1 * _rng.normal(size=(N, Q))
XS = _rng.uniform(-2.2, 2.2, size=(NS, D))
Z = X[::7][:M] + 0.05
X3 = _rng.normal(size=(N, 3))                        # inputs of another dimension, for the fit-time refusals
FIVE = ("predictive_gradients", "leave_one_out", "loo_log_predictive_density", "predict_with_covariance", "posterior_samples_f")


@contextlib.contextmanager
def recording(rec):
    """sparse_block_calls_record.recording, and: the wrappers of device_svgp and device_psi call through the same recording
    ``_call``; ``device.require_gpu`` gives the CPU device."""
    saved = (devs._call, devp._call, dev.require_gpu)
    with blocks.recording(rec):
        devs._call = devp._call = dev._call
        dev.require_gpu = lambda device=None: torch.device("cpu")
        try:
            yield rec
        finally:
            devs._call, devp._call, dev.require_gpu = saved


class Case(object):
    def __init__(self, rec):
        self.rec = rec

    def op(self, name, fn):
        self.rec.events.append(["op", name])
        try:
            fn()
        except AssertionError:
            raise
        except Exception as e:
            self.rec.events.append(["raises", type(e).__name__, str(e)])

    def call(self, gp, method, *args, **maybe):
        """``gp.method(*args)`` as an operation, with those of ``maybe`` that the method's signature has."""
        m = getattr(gp, method)
        kw = {k: v for k, v in maybe.items() if k in inspect.signature(m).parameters}
        self.op(method, lambda: m(*args, **kw))

    def five(self, gp):
        self.call(gp, "predictive_gradients", XS, budget_bytes=1)
        self.call(gp, "leave_one_out", budget_bytes=1)
        self.call(gp, "loo_log_predictive_density", budget_bytes=1)
        self.call(gp, "predict_with_covariance", XS)
        self.op("posterior_samples_f", lambda: gp.posterior_samples_f(XS, size=2, seed=7))

    def attrs(self, gp):
        for name in ("inducing_ids", "inducing_inputs", "lengthscales"):
            if hasattr(gp, name):
                v = getattr(gp, name)
                event = ["attr", name, None if v is None else list(np.shape(v))]
                if name == "inducing_ids" and v is not None:
                    event.append([int(i) for i in v])
                self.rec.events.append(event)

    def plugin(self, gp, further=()):
        """The operations of every plugin, then ``further``: (name, function of the fitted plugin) pairs."""
        self.five(gp)
        self.op("fit", lambda: gp.fit([X, Y]))
        self.attrs(gp)
        self.op("predict", lambda: gp.predict(XS))
        self.call(gp, "predict_with_variance", XS, include_noise=True, budget_bytes=1)
        self.five(gp)
        for name, fn in further:
            self.op(name, lambda: fn(gp))

    def refusals(self, cls, bad_arguments, bad_fits):
        for kw in bad_arguments:
            self.op("%s(%s)" % (cls.__name__, ", ".join("%s=%r" % kv for kv in sorted(kw.items()))), lambda: cls(**kw))
        for name, fn in bad_fits:
            self.op(name, fn)


CASES = []                      # (name, function of a Case)


def case(name, make, further=()):
    CASES.append((name, lambda c: c.plugin(make(), further)))


# ---- the sparse plugins -------------------------------------------------------------------------------------------------
SPARSE_OBJECTIVE = (
    ("log_marginal_likelihood", lambda g: g.log_marginal_likelihood()),
    ("log_marginal_likelihood_at", lambda g: g.log_marginal_likelihood(ell=0.9, sf=1.2, noise=0.05)),
    ("log_marginal_likelihood_grad", lambda g: g.log_marginal_likelihood_grad()),
    ("log_marginal_likelihood_grad_at", lambda g: g.log_marginal_likelihood_grad(ell=0.9, noise=0.05, want_z=False)),
)
LINEAR_OBJECTIVE = SPARSE_OBJECTIVE + (
    ("log_marginal_likelihood_linear", lambda g: g.log_marginal_likelihood(ell=[0.9, 1.1], linear=0.3)),
    ("log_marginal_likelihood_grad_linear", lambda g: g.log_marginal_likelihood_grad(linear=[0.3, 0.2])),
)

for _cls in (ca.SGP_FITC, ca.SparseGP_RBF):
    for _ard in (False, True):
        for _given in (False, True):
            case("%s%s_%s" % (_cls.__name__, "_ard" if _ard else "", "given_z" if _given else "drawn_z"),
                 lambda cls=_cls, ard=_ard, given=_given: cls(num_inducing=M, lengthscale=(0.7, 1.3) if ard else 0.7, variance=1.3,
                                                              Z=Z if given else None, seed=3, ARD=ard),
                 SPARSE_OBJECTIVE if _ard == _given else ())
case("SparseGP_matern32", lambda: ca.SparseGP(num_inducing=M, nu=1.5, lengthscale=0.7), SPARSE_OBJECTIVE[:1])
case("SparseGP_RBFLinear", lambda: ca.SparseGP_RBFLinear(num_inducing=M, lengthscale=(0.7, 1.3), linear_variance=(0.5, 0.2), Z=Z),
     LINEAR_OBJECTIVE)

# ---- SVIGP_RBF ------------------------------------------------------------------------------------------------------------
SVGP_OBJECTIVE = (("elbo", lambda g: g.elbo()), ("elbo_grad", lambda g: g.elbo_grad()),
                  ("elbo_grad_at", lambda g: g.elbo_grad(np.array(g.params))),
                  ("elbo_of_another_length", lambda g: g.elbo(np.zeros(3))))
for _ard in (False, True):
    for _linear in (False, True):
        case("SVIGP_RBF%s%s" % ("_ard" if _ard else "", "_linear" if _linear else ""),
             lambda ard=_ard, linear=_linear: ca.SVIGP_RBF(num_inducing=M, optimize=False, ARD=ard, linear=linear, seed=3),
             SVGP_OBJECTIVE if _ard == _linear else ())
case("SVIGP_RBF_gaussian", lambda: ca.SVIGP_RBF(num_inducing=M, optimize=False, likelihood="gaussian", Z=Z), SVGP_OBJECTIVE[:1])

# ---- BGPLVM ---------------------------------------------------------------------------------------------------------------
PSI_OBJECTIVE = (
    ("elbo", lambda g: g.elbo()), ("kl_divergence", lambda g: g.kl_divergence()),
    ("predict_test_var_scalar", lambda g: g.predict(XS, test_var=0.1, budget_bytes=1)),
    ("predict_test_var_rows", lambda g: g.predict(XS, test_var=np.full((NS, D), 0.1), budget_bytes=1)),
    ("predict_with_variance_test_var", lambda g: g.predict_with_variance(XS, test_var=0.1)),
    ("predict_test_var_of_another_shape", lambda g: g.predict(XS, test_var=np.zeros(3))),
)
for _name, _var in (("none", None), ("scalar", 0.05), ("vector", np.array([0.05, 0.0])), ("rows", np.full((N, D), 0.05))):
    case("BGPLVM_x_var_%s" % _name, lambda var=_var: ca.BGPLVM(num_inducing=M, X_var=var, seed=3),
         PSI_OBJECTIVE if _name in ("scalar", "rows") else PSI_OBJECTIVE[:2])
case("BGPLVM_isotropic", lambda: ca.BGPLVM(num_inducing=M, ARD=False, lengthscale=0.7, Z=Z), PSI_OBJECTIVE[:3])

# ---- the exact plugins ----------------------------------------------------------------------------------------------------
for _ard in (False, True):
    _lml = (("log_marginal_likelihood",
             lambda g, ard=_ard: g.log_marginal_likelihood(g.block.x, g._y, np.array([0.9, 1.1]) if ard else 0.9, 1.2, 0.05)),)
    case("GP_RBF%s" % ("_ard" if _ard else ""), lambda ard=_ard: ca.GP_RBF(lengthscale=0.7, optimize=False, ARD=ard), _lml)
    case("GP_Matern%s" % ("_ard" if _ard else ""), lambda ard=_ard: ca.GP_Matern(2.5, lengthscale=0.7, optimize=False, ARD=ard), _lml)

# ---- the optimisers (module docstring) ------------------------------------------------------------------------------------
OPTIMIZER_CASES = []


def optimizer_case(name, make):
    def fn(c):
        gp = make()
        c.op("fit", lambda: gp.fit([X, Y]))
        c.attrs(gp)
    OPTIMIZER_CASES.append((name, fn))


_opt = dict(num_inducing=M, optimize=True, max_iters=2, seed=3)
optimizer_case("optimize_SparseGP_2_point", lambda: ca.SparseGP(ARD=True, **_opt))
optimizer_case("optimize_SparseGP_analytic", lambda: ca.SparseGP(jac="analytic", **_opt))
optimizer_case("optimize_SparseGP_inducing", lambda: ca.SparseGP_RBFLinear(jac="analytic", optimize_inducing=True, **_opt))
optimizer_case("optimize_SVIGP_RBF", lambda: ca.SVIGP_RBF(**_opt))
optimizer_case("optimize_BGPLVM", lambda: ca.BGPLVM(**_opt))
CASES.extend(OPTIMIZER_CASES)

# ---- refusals: the bad constructor arguments of the host tests, and what a fit refuses ------------------------------------
_NAN, _INF = float("nan"), float("inf")
_BAD_LENGTHSCALES = [dict(lengthscale=(0.7, 1.3)), dict(lengthscale=[0.7], ARD=False), dict(lengthscale=[[0.7, 1.3]], ARD=True)] + [
    dict(lengthscale=bad, ARD=True) for bad in (0.0, -1.0, _NAN, _INF, (0.7, 0.0), (0.7, -1.3), (_NAN, 1.3), (0.7, _INF), ())]
_BAD_SPARSE = [dict(nu=2.0), dict(num_inducing=0), dict(jac="3-point"), dict(optimize_inducing=True),
               dict(optimize=True, optimize_inducing=True), dict(lengthscale=0.0), dict(variance=-1.0), dict(dtype="f16"),
               dict(jitter=-1.0), dict(num_inducing=0, jac="3-point", lengthscale=(0.7, 1.3), nu=2.0)]


def _fit(make, x=X):
    return lambda: make().fit([x, Y])


def _sparse_refusals(cls, extra=()):
    def fn(c):
        c.refusals(cls, ([dict(approximation="svgp")] if "approximation" in inspect.signature(cls.__init__).parameters else [])
                   + _BAD_SPARSE + _BAD_LENGTHSCALES + list(extra),
                   [("fit_lengthscale_of_another_length", _fit(lambda: cls(num_inducing=M, lengthscale=(0.7, 1.3), ARD=True), X3)),
                    ("fit_z_of_another_dimension", _fit(lambda: cls(num_inducing=M, Z=Z), X3)),
                    ("fit_jitter_negative", _fit(lambda: cls(num_inducing=M, jitter=-1.0)))])
    CASES.append(("refusals_%s" % cls.__name__, fn))


for _cls in (ca.SparseGP, ca.SGP_FITC, ca.SparseGP_RBF):
    _sparse_refusals(_cls)
_sparse_refusals(ca.SparseGP_RBFLinear, [dict(linear_variance=bad) for bad in (0.0, -1.0, _NAN, _INF, [0.5, 0.0], [0.5, -0.2], [0.5, _NAN],
                                                                               [], [[0.5, 0.2]])] + [dict(approximation="exact")])


def refusals_SparseGP_RBFLinear_fit(c):
    c.op("fit_linear_variance_of_another_length", _fit(lambda: ca.SparseGP_RBFLinear(num_inducing=M, linear_variance=[0.5, 0.2, 0.1])))
    gp = ca.SparseGP_RBF(num_inducing=M)
    c.op("fit", lambda: gp.fit([X, Y]))
    c.op("linear_of_a_model_without_the_term", lambda: gp.log_marginal_likelihood(linear=[0.5, 0.2]))


def refusals_SVIGP_RBF(c):
    c.refusals(ca.SVIGP_RBF,
               [dict(likelihood="laplace"), dict(num_inducing=0), dict(lengthscale=0.0), dict(lengthscale=[1.0, 2.0]), dict(variance=-1.0),
                dict(linear_variance=0.0), dict(deg_free=0.0), dict(white_variance=-0.1), dict(jitter=-1.0), dict(nu=2.0),
                dict(dtype="f16"), dict(dtype="f32"), dict(variance=_NAN), dict(white_variance=_NAN),
                dict(likelihood="laplace", num_inducing=0, lengthscale=0.0, jitter=-1.0, dtype="f32", nu=2.0)],
               [("fit_z_of_another_dimension", _fit(lambda: ca.SVIGP_RBF(num_inducing=M, Z=Z, optimize=False), X3))])
    gp = ca.SVIGP_RBF(num_inducing=M)
    for name in ("elbo", "elbo_grad"):
        c.op("%s_before_fit" % name, getattr(gp, name))
    c.op("predict_before_fit", lambda: gp.predict(XS))
    c.op("_predict_before_fit", lambda: gp._predict(XS))
    c.op("predict_with_variance_before_fit", lambda: gp.predict_with_variance(XS))


def refusals_BGPLVM(c):
    c.refusals(ca.BGPLVM,
               [dict(num_inducing=0), dict(noise=0.0), dict(noise=[1.0]), dict(variance=-1.0), dict(lengthscale=0.0),
                dict(lengthscale=[1.0, -1.0]), dict(lengthscale=[1.0, 2.0], ARD=False), dict(lengthscale=[[1.0]]), dict(jitter=-1.0),
                dict(X_var=-0.1), dict(X_var=[0.1, _NAN]), dict(X_var=np.zeros((2, 2, 2))), dict(lengthscale=[]),
                dict(num_inducing=0, noise=0.0, lengthscale=[[1.0]], jitter=-1.0, X_var=-0.1)],
               [("fit_lengthscale_of_another_length", _fit(lambda: ca.BGPLVM(num_inducing=M, lengthscale=[1.0, 2.0]), X3)),
                ("fit_z_of_another_dimension", _fit(lambda: ca.BGPLVM(num_inducing=M, Z=Z), X3)),
                ("fit_x_var_vector_of_another_length", _fit(lambda: ca.BGPLVM(num_inducing=M, X_var=[0.1, 0.1, 0.1]))),
                ("fit_x_var_rows_of_another_shape", _fit(lambda: ca.BGPLVM(num_inducing=M, X_var=np.zeros((N - 1, D)))))])
    gp = ca.BGPLVM(num_inducing=M)
    for name, args in (("predict", (XS,)), ("predict_with_variance", (XS,)), ("elbo", ()), ("kl_divergence", ())):
        c.op("%s_before_fit" % name, lambda: getattr(gp, name)(*args))
    c.op("predict_test_var_before_fit", lambda: gp.predict(XS, test_var=0.1))
    c.op("predict_with_variance_test_var_before_fit", lambda: gp.predict_with_variance(XS, test_var=0.1))


def refusals_exact(c):
    c.refusals(ca.GP_Matern, [dict(nu=2.0), dict(dtype="f16"), dict(lengthscale=0.0)], [])
    c.refusals(ca.GP_RBF, [dict(dtype="f16"), dict(lengthscale=0.0), dict(variance=-1.0)], [])
    gp = ca.GP_RBF(optimize=False)
    c.op("predict_before_fit", lambda: gp.predict(XS))
    c.op("predict_with_variance_before_fit", lambda: gp.predict_with_variance(XS))


for _fn in (refusals_SparseGP_RBFLinear_fit, refusals_SVIGP_RBF, refusals_BGPLVM, refusals_exact):
    CASES.append((_fn.__name__, _fn))


def plugin_classes():
    return [getattr(ca, name) for name in ca.__all__
            if inspect.isclass(getattr(ca, name)) and issubclass(getattr(ca, name), ca.RegressionMethod)]


def signatures():
    """{"Class.method": signature} of ``__init__`` and every public method of every exported plugin class."""
    out = {}
    for cls in plugin_classes():
        for name, f in inspect.getmembers(cls, inspect.isfunction):
            if name == "__init__" or not name.startswith("_"):
                out["%s.%s" % (cls.__name__, name)] = str(inspect.signature(f))
    return out


def run_case(fn):
    with recording(blocks.Recorder()) as rec:
        fn(Case(rec))
        return {"events": rec.events}


def run_all():
    log = {name: run_case(fn) for name, fn in CASES}
    log["signatures"] = signatures()
    return log


def calls(entry):
    return [e for e in entry["events"] if e[0] not in ("op", "read", "raises", "attr")]


if __name__ == "__main__":
    log, again = run_all(), run_all()
    for name, _ in OPTIMIZER_CASES:
        assert base.dumps(log[name]) == base.dumps(again[name]), "%s: two recordings differ, leave the case out" % name
    assert base.dumps(log) == base.dumps(again)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), base.dumps(v)) for k, v in log.items()) + "\n}\n")
    print("%d cases, %d C calls -> %s" % (len(CASES), sum(len(calls(e)) for k, e in log.items() if k != "signatures"), GOLDEN))
