"""The regression plugins' calls into the C ABI, their host read-backs, their refusals and their signatures, replayed on the
CPU against the recorded log tests/golden/plugin_calls.json, in the manner of tests/test_sparse_block_calls_host.py: for
every case of tests/plugin_calls_record.py the same C functions in the same order with the same arguments, the same reads
between them, the same exceptions with the same words, and the same attributes after a fit.  The log was written from the
commit before the plugins got their common inducing-point base."""
import json

import pytest

import device_calls_record as base
import plugin_calls_record as rec

with open(rec.GOLDEN) as f:
    LOG = json.load(f)

NAMES = [name for name, _ in rec.CASES]
INDUCING = [name for name in NAMES if name.split("_")[0] in ("SGP", "SparseGP", "SVIGP", "BGPLVM")]


def test_log_and_cases_name_the_same_entries():
    assert sorted(LOG) == sorted(NAMES + ["signatures"]) and len(set(NAMES)) == len(NAMES)


@pytest.mark.parametrize("name,fn", rec.CASES, ids=NAMES)
def test_case_replays_the_recorded_calls(name, fn):
    got, want = rec.run_case(fn), LOG[name]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert base.dumps(g) == base.dumps(w), "event %d" % k
    assert base.dumps(got) == base.dumps(want)


def test_signatures_of_the_public_methods_have_not_changed():
    got, want = rec.signatures(), LOG["signatures"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert len(want) > 90 and {name.split(".")[0] for name in want} == {cls.__name__ for cls in rec.plugin_classes()}


def _operations(entry):
    """[(operation, its events)] of one case; a case may run an operation more than once."""
    out = []
    for e in entry["events"]:
        if e[0] == "op":
            out.append((e[1], []))
        else:
            out[-1][1].append(e)
    return out


def _tails(events):
    return [e[1][3] for e in events if e[0] == "cimrgp_sparse_tail"]          # (dtype, A*, W*, rows, ..)


def test_the_log_holds_what_it_is_there_to_pin():
    """The recorded sequences themselves: an operation that is refused makes no call and reads nothing; every
    inducing-point plugin's chunked prediction (``budget_bytes=1``) ends in tails of 256 and then 44 rows, once per output
    column for the variational block and also at uncertain test inputs; the five queries are refused before and after the
    fit by the three plugins that do not build them, in the same words both times."""
    refused = 0
    for name in NAMES:
        for op, events in _operations(LOG[name]):
            if any(e[0] == "raises" for e in events) and not name.startswith("optimize_"):
                assert len(events) == 1, (name, op)
                refused += 1
    assert refused > 300
    for name in INDUCING:
        ops = _operations(LOG[name])
        chunked = [ev for op, ev in ops if op == "predict_with_variance" or op in ("predict_test_var_scalar", "predict_test_var_rows")]
        assert chunked, name
        for events in chunked:
            assert _tails(events) == ([256, 256, 44, 44] if name.startswith("SVIGP") else [256, 44]), name
        five = [(op, ev) for op, ev in ops if op in rec.FIVE]
        assert [op for op, _ in five] == list(rec.FIVE) * 2, name
        if name.split("_")[0] in ("SVIGP", "BGPLVM") or name == "SparseGP_RBFLinear":
            for (op, before), (_, after) in zip(five[:5], five[5:]):
                assert before == after and before[0][:2] == ["raises", "TypeError"], (name, op)
                assert before[0][2].startswith("%s() of " % op) and before[0][2].endswith(") is not yet supported"), (name, op)
        else:
            assert all(ev[0][:2] == ["raises", "RuntimeError"] for _, ev in five[:5]), name
            assert all(rec.calls({"events": ev}) and not [e for e in ev if e[0] == "raises"] for _, ev in five[5:]), name


@pytest.mark.parametrize("name,fn", [c for c in rec.CASES if not c[0].startswith(("optimize_", "refusals_"))],
                         ids=[n for n in NAMES if not n.startswith(("optimize_", "refusals_"))])
def test_a_fit_makes_as_many_calls_as_the_log_has(name, fn):
    """``optimize=False``: between 7 (exact) and 19 (variational) calls, and the working tree makes as many."""
    count = lambda entry: [len(rec.calls({"events": ev})) for op, ev in _operations(entry) if op == "fit"]
    want = count(LOG[name])
    assert len(want) == 1 and 7 <= want[0] <= 19 and count(rec.run_case(fn)) == want
