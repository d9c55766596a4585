"""SparseBlock's calls into the C ABI and its host read-backs, replayed on the CPU against the recorded log
tests/golden/sparse_block_calls.json, in the manner of tests/test_device_linear_calls_host.py: for every case of
tests/sparse_block_calls_record.py (the plain, ARD, linear and ARD + linear arms, FITC and VFE, a model layer's block, the
refusals) the same C functions in the same order with the same arguments and the same reads between them.  The log was
written from the commit before the block's covariance became one object."""
import json

import pytest

import device_calls_record as base
import sparse_block_calls_record as rec

with open(rec.GOLDEN) as f:
    LOG = json.load(f)

IDS = ["%s[%d]" % (name, v) for name, _ in rec.CASES for v in (0, 1)]


def test_log_and_cases_name_the_same_entries():
    assert sorted(LOG) == sorted(IDS) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("name,fn", rec.CASES, ids=[c[0] for c in rec.CASES])
@pytest.mark.parametrize("v", (0, 1))
def test_case_replays_the_recorded_calls(name, fn, v):
    got, want = rec.run_case(fn, v), LOG["%s[%d]" % (name, v)]
    for k, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert base.dumps(g) == base.dumps(w), "event %d" % k
    assert base.dumps(got) == base.dumps(want)


def _operations(entry):
    """{operation: its events} of one case."""
    out, name = {}, None
    for e in entry["events"]:
        if e[0] == "op":
            name = e[1]
            out[name] = []
        else:
            out[name].append(e)
    return out


def test_the_log_holds_what_it_is_there_to_pin():
    """The recorded sequences themselves: the refusals make no call, fit + predict + lml_grad are as many calls in every
    arm (12 + 8 + 27 under FITC: the size queries count, and the test rows go in two chunks), a layer's block reads
    nothing back, and lml_grad reads back once, at its end."""
    for name in ("ready_for_refusals[0]", "ready_for_refusals[1]"):
        ops = _operations(LOG[name])
        assert len(ops) == 12 and all(len(ev) == 1 and ev[0][0] == "raises" for ev in ops.values()), name
    for arm in ("plain", "ard", "linear", "ard_linear"):
        for approximation in ("fitc", "vfe"):
            ops = _operations(LOG["%s_%s[1]" % (arm, approximation)])
            count = lambda op: len(rec.calls({"events": ops[op]}))
            grad_calls = 27 if approximation == "fitc" else 25        # VFE has A^T diag(t) A from B: no second cimrgp_wsyrk_tn
            assert (count("fit"), count("predict"), count("lml_grad")) == (12, 8, grad_calls), (arm, approximation)
            tails = [e[1] for e in ops["predict"] if e[0] == "cimrgp_sparse_tail"]
            assert [t[3] for t in tails] == [256, 44]                 # (dtype, A*, W*, rows, ..)
            grad = ops["lml_grad"]
            reads = [k for k, e in enumerate(grad) if e[0] == "read"]
            assert reads == [len(grad) - 1] and grad[-1][1] == "cpu", (arm, approximation)
            assert [e[1] for e in ops["fit"] if e[0] == "read"] == ["item"] * 3
    for name in ("layer_fitc_noise_from_the_targets[0]", "layer_vfe_noise_fixed[1]"):
        ops = _operations(LOG[name])
        assert not [e for op in ("fit_layer", "fit_layer_shared", "predict_layer") for e in ops[op] if e[0] in ("read", "raises")]
        refusal = "predict_grad() of a sparse layer of the model (device_noise=True) is not yet supported"
        assert ops["predict_grad_refused"] == [["raises", "TypeError", refusal]]
