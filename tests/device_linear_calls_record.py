"""Every C call of cimrgp_amd/device_linear.py, recorded on the CPU with the recorder of tests/device_calls_record.py (its
stand-in library, its two variants per case, its event format): shared by tests/test_device_linear_calls_host.py, which
replays the cases below and compares with tests/golden/device_linear_calls.json.  Run as a script
(``python tests/device_linear_calls_record.py``) it writes that file.  device_linear's wrappers allocate and call through
``device``'s helpers, which the recorder patches, so nothing here is patched again."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import device_calls_record as base  # noqa: E402
from cimrgp_amd import device_linear as devl  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "device_linear_calls.json")
N, NS, M, D = base.N, base.NS, base.M, base.D

CASES = []                      # (name, function, refused)


def case(fn):
    CASES.append((fn.__name__, fn, False))
    return fn


def refused(fn):
    CASES.append((fn.__name__, fn, True))
    return fn


def _lin(c, d=D, name="lin"):
    return c.t(name, d, dtype=torch.float64, view=False)


@case
def cov_gram_lin(c):
    x = c.t("x", N, D)
    return devl.cov_gram_lin(x, c.x(0.7), 1.3, _lin(c), 0.01, lower_only=c.flag, out=None if not c.v else c.mat("k", N, N), cov=c.cov)


@case
def cov_cross_lin(c):
    xa, xb = c.t("xa", NS, D), c.t("xb", N, D)
    return devl.cov_cross_lin(xa, xb, 0.7, c.x(1.5), _lin(c), out=None if not c.v else c.mat("kab", NS, N), cov=c.cov)


@refused
def cov_cross_lin_weights_of_another_dtype(c):
    xa, xb = c.t("xa", NS, D), c.t("xb", N, D)
    lin = c.t("lin", D, dtype=torch.float32, view=False) if c.v else _lin(c, D + 1)
    return devl.cov_cross_lin(xa, xb, 0.7, 1.5, lin)


@case
def sparse_lambda_kd(c):
    a = c.mat("a", N, M)
    kd = c.t("kdiag", N, view=False)
    return devl.sparse_lambda_kd(a, c.n(N), c.n(M), kd, c.x(0.05), c.n(c.v), lam=c.opt("lam", N), w=c.opt("w", N),
                                 sums=c.opt("sums", 3, dtype=torch.float64))


@refused
def sparse_lambda_kd_diagonal_refused(c):
    a = c.mat("a", N, M)
    kd = c.t("kdiag", N, dtype=torch.float32, view=False) if c.v else c.t("kdiag", N - 1, view=False)
    return devl.sparse_lambda_kd(a, N, M, kd, 0.05, 0)


@case
def cov_pair_grad_lin(c):
    xa, xb, g = c.t("xa", N, D), c.t("xb", M, D), c.mat("g", N, M)
    nsums = 1 + D if c.v else 2
    out = [devl.cov_pair_grad_lin_scratch_bytes(c.n(N), c.n(M), c.n(D), c.flag)]
    out.append(devl.cov_pair_grad_lin(xa, xb, g, c.x(0.7), 1.3, _lin(c), ard=c.flag, scale=c.x(2.0), accumulate=c.flag,
                                      sums=c.opt("sums", nsums, dtype=torch.float64), lsums=c.opt("lsums", D, dtype=torch.float64),
                                      db=c.opt("db", M, D), cov=c.cov, scratch=None if not c.v else c.ws("scratch", 1 << 16)))
    # an output that is not wanted is neither allocated nor passed, given or not
    out.append(devl.cov_pair_grad_lin(xa, xb, g, 0.7, 1.3, _lin(c, name="lin2"), want_sums=bool(c.v), want_lsums=not c.v, want_db=not c.v,
                                      sums=c.opt("sums2", 2, dtype=torch.float64), lsums=c.opt("lsums2", D, dtype=torch.float64),
                                      db=c.opt("db2", M, D)))
    return out


@refused
def unknown_covariance(c):
    x = c.t("x", N, D)
    return devl.cov_gram_lin(x, 0.7, 1.3, _lin(c), cov=4 if c.v else -1)


def run_case(fn, v):
    return base.run_case(fn, v)


def run_all():
    return {"%s[%d]" % (name, v): run_case(fn, v) for name, fn, _ in CASES for v in (0, 1)}


if __name__ == "__main__":
    log = run_all()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), base.dumps(v)) for k, v in log.items()) + "\n}\n")
    print("%d cases, %d C calls -> %s" % (len(log), sum(1 for e in log.values() for ev in e["events"] if ev[0] != "alloc"), GOLDEN))
