"""The guarded-buffer helper of tests/test_gpu_buffer_contract.py on CPU tensors: it must catch a write into a guard,
a write into a gap, a change to a const input and a NaN that leaks into an output -- otherwise the GPU file could
pass without checking anything."""
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_buffer_contract import CONST, INOUT, JUNK, OUT, Guarded, run_contract  # noqa: E402


def _bufs():
    """A 4 x 5 matrix at ld 8 with two rows below it, a two-block arena with a gap, a const vector."""
    m = Guarded("M", 6 * 8, torch.float64, "cpu", ld=8).mark(OUT, 4, 5, part="lower").mark(JUNK, 4, 5, part="upper")
    a = Guarded("arena", 2 * 12, torch.float32, "cpu")
    a.vec(INOUT, 10, off=0, values=torch.arange(10.0)).vec(INOUT, 10, off=12, values=torch.arange(10.0))
    c = Guarded("c", 5, torch.float64, "cpu").vec(CONST, 5, values=torch.linspace(0, 1, 5))
    return m, a, c


def _good(m, a, c):
    """Writes exactly its footprint; reads only const values."""
    mat = m.mat(4, 5)
    mat.copy_(torch.tril(c.data[:5].repeat(4, 1) + 1.0))
    mat.add_(torch.triu(torch.full((4, 5), 3.0, dtype=torch.float64), 1))     # junk above the diagonal is allowed
    for off in (0, 12):
        a.data[off:off + 10] += 2.0


def test_a_correct_call_passes():
    m, a, c = _bufs()
    run_contract([m, a, c], lambda: _good(m, a, c))
    assert float(m.mat(4, 5)[3, 0]) == 1.0 and float(a.data[13]) == 3.0


def test_a_write_into_a_guard_is_caught():
    m, a, c = _bufs()
    with pytest.raises(AssertionError, match="guard after"):
        run_contract([m, a, c], lambda: (_good(m, a, c), m.full[-1].fill_(1.0)))
    with pytest.raises(AssertionError, match="guard before"):
        run_contract([m, a, c], lambda: (_good(m, a, c), a.full[a.g - 1].fill_(1.0)))


def test_a_write_into_padding_or_a_gap_is_caught():
    m, a, c = _bufs()
    with pytest.raises(AssertionError, match="row 2, column 5"):
        run_contract([m, a, c], lambda: (_good(m, a, c), m.data[2 * 8 + 5].fill_(0.0)))
    with pytest.raises(AssertionError, match="arena"):
        run_contract([m, a, c], lambda: (_good(m, a, c), a.data[11].fill_(0.0)))


def test_a_change_to_a_const_input_is_caught():
    m, a, c = _bufs()
    with pytest.raises(AssertionError, match="c: 1 element"):
        run_contract([m, a, c], lambda: (_good(m, a, c), c.data[4].mul_(1.0 + 1e-15)))


def test_a_nan_leaking_into_an_output_is_caught():
    m, a, c = _bufs()

    def reads_padding():                 # multiplies the unread padding by zero: only the NaN run shows it
        _good(m, a, c)
        m.mat(4, 5)[1, 0] += 0.0 * m.data[1 * 8 + 6]
    with pytest.raises(AssertionError, match="nan run differ"):
        run_contract([m, a, c], reads_padding)

    def reads_old_output():              # uses what the output held before the call: the random run shows it
        old = m.mat(4, 5)[2, 1].clone()
        _good(m, a, c)
        m.mat(4, 5)[2, 1] += torch.nan_to_num(old, nan=0.0)
    with pytest.raises(AssertionError, match="rand run differ"):
        run_contract([m, a, c], reads_old_output)
