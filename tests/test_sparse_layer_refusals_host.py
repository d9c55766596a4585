"""Every refusal of include/cimrgp_sparse_layer.h that comes before any HIP call, pinned as a literal table in the manner of
tests/test_sparse_refusals_host.py: entry point, arguments, status and the full cimrgp_last_error() text.  No GPU is needed
and no row launches anything.  Also: the header's symbols are exported and registered."""
import os
import re

import pytest

from cimrgp_amd import _lib
from test_sparse_refusals_host import _stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = {
    'cimrgp_sparse_lambda_dev': [('dtype', 1), ('a', 'P'), ('n', 600), ('m', 100), ('lda', 112), ('sf2', 1.0), ('noise', 'P'),
        ('mode', 0), ('lam', 'P'), ('w', 'P'), ('sums', 'P'), ('stream', None)],
    'cimrgp_sparse_tail_dev': [('dtype', 1), ('astar', 'P'), ('wstar', 'P'), ('ns', 50), ('m', 100), ('lda', 112), ('gamma', 'P'),
        ('q', 2), ('sf2', 1.0), ('extra_var', 0.0), ('bias', 'P'), ('extra_var_dev', 'P'), ('mean', 'P'), ('var', 'P'),
        ('accumulate', 0), ('stream', None)],
}

ROWS = [
    ('cimrgp_sparse_lambda_dev', {'dtype': 7}, -1, 'cimrgp_sparse_lambda_dev: unknown dtype'),
    ('cimrgp_sparse_lambda_dev', {'a': None}, -1, 'cimrgp_sparse_lambda_dev: null pointer'),
    ('cimrgp_sparse_lambda_dev', {'lam': None}, -1, 'cimrgp_sparse_lambda_dev: null pointer'),
    ('cimrgp_sparse_lambda_dev', {'w': None}, -1, 'cimrgp_sparse_lambda_dev: null pointer'),
    ('cimrgp_sparse_lambda_dev', {'sums': None}, -1, 'cimrgp_sparse_lambda_dev: null pointer'),
    ('cimrgp_sparse_lambda_dev', {'noise': None}, -1, 'cimrgp_sparse_lambda_dev: null pointer (noise)'),
    ('cimrgp_sparse_lambda_dev', {'n': 0}, -1, 'cimrgp_sparse_lambda_dev: bad dimensions'),
    ('cimrgp_sparse_lambda_dev', {'n': 1 << 31}, -1, 'cimrgp_sparse_lambda_dev: bad dimensions'),
    ('cimrgp_sparse_lambda_dev', {'m': 0}, -1, 'cimrgp_sparse_lambda_dev: bad dimensions'),
    ('cimrgp_sparse_lambda_dev', {'lda': 99}, -1, 'cimrgp_sparse_lambda_dev: bad dimensions'),
    ('cimrgp_sparse_lambda_dev', {'mode': 2}, -1, 'cimrgp_sparse_lambda_dev: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda_dev', {'mode': -1}, -1, 'cimrgp_sparse_lambda_dev: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda_dev', {'dtype': 7, 'a': None, 'noise': None, 'n': 0, 'mode': 2}, -1,
     'cimrgp_sparse_lambda_dev: unknown dtype'),
    ('cimrgp_sparse_lambda_dev', {'a': None, 'noise': None, 'n': 0}, -1, 'cimrgp_sparse_lambda_dev: null pointer'),
    ('cimrgp_sparse_tail_dev', {'dtype': 7}, -1, 'cimrgp_sparse_tail_dev: unknown dtype'),
    ('cimrgp_sparse_tail_dev', {'wstar': None}, -1, 'cimrgp_sparse_tail_dev: null pointer'),
    ('cimrgp_sparse_tail_dev', {'astar': None}, -1, 'cimrgp_sparse_tail_dev: null pointer (astar)'),
    ('cimrgp_sparse_tail_dev', {'gamma': None}, -1, 'cimrgp_sparse_tail_dev: null pointer (gamma)'),
    ('cimrgp_sparse_tail_dev', {'ns': -1}, -1, 'cimrgp_sparse_tail_dev: bad dimensions'),
    ('cimrgp_sparse_tail_dev', {'ns': 1 << 31}, -1, 'cimrgp_sparse_tail_dev: bad dimensions'),
    ('cimrgp_sparse_tail_dev', {'m': 0}, -1, 'cimrgp_sparse_tail_dev: bad dimensions'),
    ('cimrgp_sparse_tail_dev', {'lda': 99}, -1, 'cimrgp_sparse_tail_dev: bad dimensions'),
    ('cimrgp_sparse_tail_dev', {'q': 0}, -1, 'cimrgp_sparse_tail_dev: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_tail_dev', {'q': 9}, -1, 'cimrgp_sparse_tail_dev: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_tail_dev', {'dtype': 7, 'wstar': None, 'astar': None, 'gamma': None, 'ns': -1, 'q': 0}, -1,
     'cimrgp_sparse_tail_dev: unknown dtype'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [
    ('cimrgp_sparse_tail_dev', {'ns': 0}),
    ('cimrgp_sparse_tail_dev', {'ns': 0, 'bias': None, 'extra_var_dev': None}),
    ('cimrgp_sparse_tail_dev', {'mean': None, 'var': None, 'astar': None, 'gamma': None, 'q': 0}),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def test_sparse_layer_header_symbols_are_exported_and_registered():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "cimrgp_sparse_layer.h")).read()
    names = sorted(set(re.findall(r"^(?:int|size_t)\s+(cimrgp_\w+)\s*\(", text, re.M)))
    assert names == ["cimrgp_sparse_lambda_dev", "cimrgp_sparse_tail_dev"] == sorted(_lib.SPARSE_LAYER_SIGNATURES) == sorted(BASE)
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SPARSE_LAYER_SIGNATURES[name][1], name
        assert len(BASE[name]) == len(_lib.SPARSE_LAYER_SIGNATURES[name][1]), name
    assert '#include "cimrgp_sparse_layer.h"' in open(os.path.join(ROOT, "include", "cimrgp.h")).read()
    assert {row[0] for row in ROWS} == set(BASE)
    # each is its twin with the new arguments in place: same argument count but for the two new pointers of the tail
    assert len(_lib.SPARSE_LAYER_SIGNATURES["cimrgp_sparse_lambda_dev"][1]) == len(_lib.SPARSE_SIGNATURES["cimrgp_sparse_lambda"][1])
    assert len(_lib.SPARSE_LAYER_SIGNATURES["cimrgp_sparse_tail_dev"][1]) == len(_lib.SPARSE_SIGNATURES["cimrgp_sparse_tail"][1]) + 2


@pytest.mark.parametrize("name", sorted(BASE))
def test_sparse_layer_refusals_status_and_text(name):
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE[name]]
    for _, broken, status, text in [row for row in ROWS if row[0] == name]:
        assert broken and set(broken) <= set(keys), broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_sparse_layer_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name, broken in NO_WORK:
        assert getattr(lib, name)(*_args(name, broken, stand_in)) == 0, (name, broken)
