"""device.py's calls into the C ABI, replayed on the CPU against the recorded log tests/golden/device_calls.json: for
every case of tests/device_calls_record.py the same C functions in the same order with the same arguments (scalars by
type and value, pointers by tensor and byte offset), the same allocations (kind, shape, dtype) between them, the same
return value and the same Python-side refusal.  The log was recorded before device.py's calls went through one
marshalling helper; no entry of it is edited by hand."""
import inspect
import json
import re

import pytest

import device_calls_record as rec
from cimrgp_amd import device as dev

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
        assert rec.dumps(g) == rec.dumps(w), "event %d" % k
    assert rec.dumps(got) == rec.dumps(want)
    if refused:         # a refusal comes before any allocation and any call
        assert got["events"] == [] and "raises" in got and "returns" not in got


def test_every_wrapper_that_reaches_the_library_has_a_case():
    """Each C function device.py names is called by some case, and each public function of device.py that names one is
    named by the cases' source."""
    called = {e[0] for entry in LOG.values() for e in entry["events"] if e[0] != "alloc"}
    source = inspect.getsource(dev)
    named = set(re.findall(r'"(cimrgp_\w+)"', source)) | set(re.findall(r"\.(cimrgp_\w+)\(", source))
    assert named and named <= called, sorted(named - called)
    cases = inspect.getsource(rec)
    for fname, f in inspect.getmembers(dev, inspect.isfunction):
        if f.__module__ == dev.__name__ and not fname.startswith("_") and re.search(r'"cimrgp_\w+"|\.cimrgp_\w+\(', inspect.getsource(f)):
            assert "dev.%s" % fname in cases, fname
