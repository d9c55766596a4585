"""device_linear.py's calls into the C ABI, replayed on the CPU against the recorded log
tests/golden/device_linear_calls.json, in the manner of tests/test_device_calls_host.py: for every case of
tests/device_linear_calls_record.py the same C functions in the same order with the same arguments, the same allocations
between them, the same return value and the same Python-side refusal."""
import inspect
import json
import re

import pytest

import device_calls_record as base
import device_linear_calls_record as rec
from cimrgp_amd import _lib, device_linear as devl

with open(rec.GOLDEN) as f:
    LOG = json.load(f)

IDS = ["%s[%d]" % (name, v) for name, _, _ in rec.CASES for v in (0, 1)]


def test_log_and_cases_name_the_same_entries():
    assert sorted(LOG) == sorted(IDS) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("name,fn,refused", rec.CASES, ids=[c[0] for c in rec.CASES])
@pytest.mark.parametrize("v", (0, 1))
def test_case_replays_the_recorded_calls(name, fn, refused, v):
    got, want = rec.run_case(fn, v), LOG["%s[%d]" % (name, v)]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert base.dumps(g) == base.dumps(w), "event %d" % k
    assert base.dumps(got) == base.dumps(want)
    if refused:         # a refusal comes before any allocation and any call
        assert got["events"] == [] and "raises" in got and "returns" not in got


def test_every_wrapper_has_a_case_and_every_symbol_is_called():
    called = {e[0] for entry in LOG.values() for e in entry["events"] if e[0] != "alloc"}
    source = inspect.getsource(devl)
    named = set(re.findall(r'"(cimrgp_\w+)"', source))
    assert named == set(_lib.SPARSE_LINEAR_SIGNATURES) and named <= called, sorted(named ^ called)
    cases = inspect.getsource(rec)
    for fname, f in inspect.getmembers(devl, inspect.isfunction):
        if f.__module__ == devl.__name__ and not fname.startswith("_"):
            assert "devl.%s" % fname in cases, fname


def test_each_wrapper_is_one_call():
    """A wrapper reaches C once, through device._call (the scratch query through device._size)."""
    for fname, f in inspect.getmembers(devl, inspect.isfunction):
        if f.__module__ == devl.__name__ and not fname.startswith("_"):
            src = inspect.getsource(f)
            assert len(re.findall(r"\b_call\(|\b_size\(", src)) == 1 or fname == "cov_pair_grad_lin", fname
    src = inspect.getsource(devl.cov_pair_grad_lin)
    assert len(re.findall(r"\b_call\(", src)) == 1
