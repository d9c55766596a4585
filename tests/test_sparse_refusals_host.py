"""Every refusal of include/cimrgp_sparse.h that comes before any HIP call, pinned as a literal table in the manner of
tests/test_abi_refusals_host.py: entry point, arguments, status and the full cimrgp_last_error() text.  No GPU is needed
and no row launches anything.  cimrgp_wsyrk_tn_scratch_bytes is a size query (0 for what it does not accept:
tests/test_sparse_host.py)."""
import ctypes

import pytest

from cimrgp_amd import _lib

BASE = {
    'cimrgp_wsyrk_tn': [('dtype', 1), ('a', 'P'), ('n', 600), ('m', 100), ('lda', 112), ('w', 'P'), ('r', 'P'), ('q', 2),
        ('diag_add', 1.0), ('c', 'P'), ('ldc', 112), ('g', 'P'), ('scratch', 'P'), ('scratch_bytes', 1 << 22), ('stream', None)],
    'cimrgp_sparse_lambda': [('dtype', 1), ('a', 'P'), ('n', 600), ('m', 100), ('lda', 112), ('sf2', 1.0), ('noise', 0.01),
        ('mode', 0), ('lam', 'P'), ('w', 'P'), ('sums', 'P'), ('stream', None)],
    'cimrgp_sparse_tail': [('dtype', 1), ('astar', 'P'), ('wstar', 'P'), ('ns', 50), ('m', 100), ('lda', 112), ('gamma', 'P'),
        ('q', 2), ('sf2', 1.0), ('extra_var', 0.0), ('mean', 'P'), ('var', 'P'), ('accumulate', 0), ('stream', None)],
}

ROWS = [
    ('cimrgp_wsyrk_tn', {'dtype': 7}, -1, 'cimrgp_wsyrk_tn: unknown dtype'),
    ('cimrgp_wsyrk_tn', {'a': None}, -1, 'cimrgp_wsyrk_tn: null pointer'),
    ('cimrgp_wsyrk_tn', {'w': None}, -1, 'cimrgp_wsyrk_tn: null pointer'),
    ('cimrgp_wsyrk_tn', {'c': None}, -1, 'cimrgp_wsyrk_tn: null pointer'),
    ('cimrgp_wsyrk_tn', {'scratch': None}, -1, 'cimrgp_wsyrk_tn: null pointer'),
    ('cimrgp_wsyrk_tn', {'g': None}, -1, 'cimrgp_wsyrk_tn: null pointer (g)'),
    ('cimrgp_wsyrk_tn', {'n': 0}, -1, 'cimrgp_wsyrk_tn: n must be in [1, 16777216]'),
    ('cimrgp_wsyrk_tn', {'n': (1 << 24) + 1}, -1, 'cimrgp_wsyrk_tn: n must be in [1, 16777216]'),
    ('cimrgp_wsyrk_tn', {'m': 0, 'lda': 16}, -1, 'cimrgp_wsyrk_tn: m must be in [1, 16384]'),
    ('cimrgp_wsyrk_tn', {'m': 16385, 'lda': 16400, 'ldc': 16400}, -1, 'cimrgp_wsyrk_tn: m must be in [1, 16384]'),
    ('cimrgp_wsyrk_tn', {'q': 0}, -1, 'cimrgp_wsyrk_tn: number of outputs must be in [1, 8]'),
    ('cimrgp_wsyrk_tn', {'q': 9}, -1, 'cimrgp_wsyrk_tn: number of outputs must be in [1, 8]'),
    ('cimrgp_wsyrk_tn', {'lda': 98}, -1, 'cimrgp_wsyrk_tn: leading dimension too small'),
    ('cimrgp_wsyrk_tn', {'ldc': 99}, -1, 'cimrgp_wsyrk_tn: leading dimension too small'),
    ('cimrgp_wsyrk_tn', {'lda': 101}, -1, 'cimrgp_wsyrk_tn: lda must be a multiple of 16 bytes'),
    ('cimrgp_wsyrk_tn', {'dtype': 0, 'lda': 102}, -1, 'cimrgp_wsyrk_tn: lda must be a multiple of 16 bytes'),
    ('cimrgp_wsyrk_tn', {'a': 'P+8'}, -1, 'cimrgp_wsyrk_tn: pointers must be 16-byte aligned'),
    ('cimrgp_wsyrk_tn', {'scratch': 'P+8'}, -1, 'cimrgp_wsyrk_tn: pointers must be 16-byte aligned'),
    ('cimrgp_wsyrk_tn', {'scratch_bytes': 417791}, -1, 'cimrgp_wsyrk_tn: scratch too small'),
    ('cimrgp_wsyrk_tn', {'r': None, 'g': None, 'q': 0, 'scratch_bytes': 393215}, -1, 'cimrgp_wsyrk_tn: scratch too small'),
    ('cimrgp_wsyrk_tn', {'dtype': 7, 'a': None, 'g': None, 'n': 0, 'm': 0, 'q': 0, 'lda': 1, 'scratch_bytes': 0}, -1,
     'cimrgp_wsyrk_tn: unknown dtype'),
    ('cimrgp_wsyrk_tn', {'a': None, 'g': None, 'n': 0}, -1, 'cimrgp_wsyrk_tn: null pointer'),
    ('cimrgp_sparse_lambda', {'dtype': 7}, -1, 'cimrgp_sparse_lambda: unknown dtype'),
    ('cimrgp_sparse_lambda', {'a': None}, -1, 'cimrgp_sparse_lambda: null pointer'),
    ('cimrgp_sparse_lambda', {'lam': None}, -1, 'cimrgp_sparse_lambda: null pointer'),
    ('cimrgp_sparse_lambda', {'w': None}, -1, 'cimrgp_sparse_lambda: null pointer'),
    ('cimrgp_sparse_lambda', {'sums': None}, -1, 'cimrgp_sparse_lambda: null pointer'),
    ('cimrgp_sparse_lambda', {'n': 0}, -1, 'cimrgp_sparse_lambda: bad dimensions'),
    ('cimrgp_sparse_lambda', {'n': 1 << 31}, -1, 'cimrgp_sparse_lambda: bad dimensions'),
    ('cimrgp_sparse_lambda', {'m': 0}, -1, 'cimrgp_sparse_lambda: bad dimensions'),
    ('cimrgp_sparse_lambda', {'lda': 99}, -1, 'cimrgp_sparse_lambda: bad dimensions'),
    ('cimrgp_sparse_lambda', {'mode': 2}, -1, 'cimrgp_sparse_lambda: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda', {'mode': -1}, -1, 'cimrgp_sparse_lambda: mode must be 0 (FITC) or 1 (VFE)'),
    ('cimrgp_sparse_lambda', {'dtype': 7, 'a': None, 'n': 0, 'mode': 2}, -1, 'cimrgp_sparse_lambda: unknown dtype'),
    ('cimrgp_sparse_tail', {'dtype': 7}, -1, 'cimrgp_sparse_tail: unknown dtype'),
    ('cimrgp_sparse_tail', {'wstar': None}, -1, 'cimrgp_sparse_tail: null pointer'),
    ('cimrgp_sparse_tail', {'astar': None}, -1, 'cimrgp_sparse_tail: null pointer (astar)'),
    ('cimrgp_sparse_tail', {'gamma': None}, -1, 'cimrgp_sparse_tail: null pointer (gamma)'),
    ('cimrgp_sparse_tail', {'ns': -1}, -1, 'cimrgp_sparse_tail: bad dimensions'),
    ('cimrgp_sparse_tail', {'ns': 1 << 31}, -1, 'cimrgp_sparse_tail: bad dimensions'),
    ('cimrgp_sparse_tail', {'m': 0}, -1, 'cimrgp_sparse_tail: bad dimensions'),
    ('cimrgp_sparse_tail', {'lda': 99}, -1, 'cimrgp_sparse_tail: bad dimensions'),
    ('cimrgp_sparse_tail', {'q': 0}, -1, 'cimrgp_sparse_tail: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_tail', {'q': 9}, -1, 'cimrgp_sparse_tail: number of outputs must be in [1, 8]'),
    ('cimrgp_sparse_tail', {'dtype': 7, 'wstar': None, 'astar': None, 'gamma': None, 'ns': -1, 'q': 0}, -1,
     'cimrgp_sparse_tail: unknown dtype'),
]

#: calls that pass every check and have nothing to do: status 0 without a launch
NO_WORK = [
    ('cimrgp_sparse_tail', {'ns': 0}),
    ('cimrgp_sparse_tail', {'mean': None, 'var': None, 'astar': None, 'gamma': None, 'q': 0}),
]


def _args(name, broken, stand_in):
    args = [broken.get(k, v) for k, v in BASE[name]]
    return [stand_in.get(a, a) if isinstance(a, str) else a for a in args]


def _stand_in():
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    return buf, {"P": p, "P+8": p + 8}


def test_every_sparse_entry_point_that_can_refuse_has_rows():
    assert set(BASE) | {"cimrgp_wsyrk_tn_scratch_bytes"} == set(_lib.SPARSE_SIGNATURES)
    assert {row[0] for row in ROWS} == set(BASE)
    for name, base in BASE.items():
        assert len(base) == len(_lib.SPARSE_SIGNATURES[name][1]), name


@pytest.mark.parametrize("name", sorted(BASE))
def test_sparse_refusals_status_and_text(name):
    lib = _lib.load()
    buf, stand_in = _stand_in()
    keys = [k for k, _ in BASE[name]]
    for _, broken, status, text in [row for row in ROWS if row[0] == name]:
        assert broken and set(broken) <= set(keys), broken
        rc = getattr(lib, name)(*_args(name, broken, stand_in))
        print(name, broken, rc, _lib.last_error())
        assert (rc, _lib.last_error()) == (status, text), (name, broken)


def test_sparse_calls_with_nothing_to_do_return_zero():
    lib = _lib.load()
    buf, stand_in = _stand_in()
    for name, broken in NO_WORK:
        assert getattr(lib, name)(*_args(name, broken, stand_in)) == 0, (name, broken)
