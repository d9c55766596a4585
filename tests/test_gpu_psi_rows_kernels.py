"""GPU tests of cimrgp_psi2_rows_quad (include/cimrgp_psi_rows.h; DESIGN.md, "Predictive variance at uncertain test
inputs") against the longdouble oracle of tests/psi_rows_numpy.py entry by entry at a bound that counts roundings
(``psi_rows_numpy.rows_quad(bound=True)`` with ``psi_grad_numpy.grad_bound``), then repeatability, the independence of a
row from n and from its place, the bad rows, the scratch size and the buffer footprint (the helper of
tests/test_gpu_buffer_contract.py).  The problems are those of tests/test_gpu_psi_kernels.py."""
import functools

import numpy as np
import pytest

import psi_grad_numpy as pg
import psi_numpy as po
import psi_rows_numpy as pr
from test_gpu_buffer_contract import CONST, CUDA, JUNK, OUT, Guarded, run_contract, wide_ld
from test_gpu_psi_kernels import ELLS, SF, SHAPES as PSI_SHAPES, TDT, UNIT, _bits, _dev, _ell_dev, _f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
#: m = 321 is the smallest m whose 21 tiles fall into groups of two with a ragged last one (11 groups; asserted below): the
#: shapes of the psi kernels have at most 6 tiles, one per group
GROUPED = (64, 321, 2)
SHAPES = list(PSI_SHAPES) + [GROUPED]
QMAX = 3
KEYS = ("tr", "quad")


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


@functools.lru_cache(maxsize=None)
def _case(n, m, d, seed=0):
    """The problem of a shape (the inputs of tests/test_gpu_psi_kernels.py), a random symmetric c and a random a with QMAX
    columns (float32-representable), the longdouble values and the bound's weights, once.  A call with q < QMAX columns
    of a has the first q columns of quad."""
    mu, s, z, _ = po.problem(n, m, d, 100 * n + m + seed, ell0=ELLS[0])
    mu, s, z = _f32(mu), _f32(s), _f32(z)
    ell = np.array(ELLS[:d])
    rng = np.random.RandomState(13 * n + m + seed)
    c = rng.randn(m, m)
    c, a = _f32(c + c.T), _f32(rng.randn(m, QMAX))
    ref = (pr.rows_quad(mu, s, z, ell, SF, c, a, LD), pr.rows_quad(mu, s, z, ell, SF, c, a, LD, bound=True))
    return dict(mu=mu, s=s, z=z, ell=ell, c=c, a=a, ref=ref)


def _weights(ca, c, q, dt):
    """c with NaN above its diagonal in a padded pitch; the first q columns of a in a wider pitch padded with NaN."""
    m = c["c"].shape[0]
    cw = torch.full((m, ca.device.padded_ld(m)), float("nan"), dtype=TDT[dt], device="cuda")
    cw[:, :m] = torch.tril(_dev(c["c"], dt)) + torch.triu(torch.full((m, m), float("nan"), dtype=TDT[dt], device="cuda"), 1)
    aw = torch.full((m, q + 5), float("nan"), dtype=TDT[dt], device="cuda")
    aw[:, :q] = _dev(c["a"][:, :q], dt)
    return cw, aw[:, :q]


def _ratios(tr, quad, ref, u, q, rows=None):
    """{key: max |got - ref| / bound} over ``rows`` (all of them if None), every entry finite (asserted)."""
    val, wts = ref
    got = dict(tr=tr.double().cpu().numpy(), quad=quad.double().cpu().numpy())
    out = {}
    for k in KEYS:
        cut = (lambda x: x) if k == "tr" else (lambda x: x[:, :q])
        v, w = cut(val[k]), tuple(cut(x) if isinstance(x, np.ndarray) else x for x in wts[k])
        ratio = np.asarray(np.abs(np.asarray(got[k], dtype=LD) - v) / pg.grad_bound(v, w, u), dtype=np.float64)
        g = got[k]
        if rows is not None:
            ratio, g = ratio[rows], g[rows]
        assert np.isfinite(g).all(), k
        out[k] = float(ratio.max())
    return out


def _show(what, ratios):
    print("%s: err/bound %s" % (what, "  ".join("%s %.3f" % (k, ratios[k]) for k in KEYS)))
    return max(ratios.values())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, QMAX])
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_rows_quad_matches_the_longdouble_oracle(ca, dt, q, n, m, d):
    """Every entry of tr and quad: |got - ref| <= grad_bound (tests/psi_rows_numpy.py has the counting); two calls give the
    same bits; no row is bad; the scratch size is the oracle's restatement of the header's rule."""
    from cimrgp_amd import device_psi as devp
    c, u = _case(n, m, d), UNIT[dt]
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    cw, aw = _weights(ca, c, q, dt)
    tr, quad, bad = devp.psi2_rows_quad(mu, s, z, ell, SF, cw, aw)
    tr2, quad2, _ = devp.psi2_rows_quad(mu, s, z, ell, SF, cw, aw)
    assert tuple(tr.shape) == (n,) and tuple(quad.shape) == (n, q)
    assert torch.equal(_bits(tr), _bits(tr2)) and torch.equal(_bits(quad), _bits(quad2))
    assert float(bad.item()) == 0.0
    assert _show("rows_quad %s q=%d (%d, %d, %d)" % (dt, q, n, m, d), _ratios(tr, quad, c["ref"], u, q)) <= 1.0
    assert devp.psi2_rows_quad_scratch_bytes(n, m, d, q, TDT[dt]) == pr.scratch_bytes(8 if dt == "f64" else 4, n, m, d, q)
    if (n, m, d) == GROUPED:
        groups, per, tiles = pr.group_rule(m)
        assert groups == 11 and groups >= 3 and tiles % per != 0                  # m alone: several groups, the last one ragged
        assert all(pr.group_rule(k)[2] % pr.group_rule(k)[1] == 0 or pr.group_rule(k)[0] < 3 for k in range(1, m))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, QMAX])
def test_a_row_does_not_depend_on_n_or_its_place(ca, dt, q):
    """The (300, 65, 3) call against a call on its rows [0, 100) alone and one on its rows [37, 137) (other row blocks, other
    threads): every row of either has the bits it has in the whole call, so chunked prediction does not depend on the
    chunking."""
    from cimrgp_amd import device_psi as devp
    n, m, d = 300, 65, 3
    c = _case(n, m, d)
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    cw, aw = _weights(ca, c, q, dt)
    tr, quad, _ = devp.psi2_rows_quad(mu, s, z, ell, SF, cw, aw)
    for a, b in ((0, 100), (37, 137)):
        ptr, pquad, _ = devp.psi2_rows_quad(mu[a:b].contiguous(), s[a:b].contiguous(), z, ell, SF, cw, aw)
        assert torch.equal(_bits(ptr), _bits(tr[a:b])) and torch.equal(_bits(pquad), _bits(quad[a:b])), (a, b)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,d", [(300, 65, 3), (150, 40, 2)])
def test_bad_rows_are_counted_and_zeroed_and_change_no_other_row(ca, dt, n, m, d):
    """Two planted rows (a negative and a NaN variance): bad = 2, their outputs are zeros, every other row keeps its bits."""
    from cimrgp_amd import device_psi as devp
    rows, q = [n // 3, n - 2], QMAX
    c = _case(n, m, d)
    s_bad = c["s"].copy()
    s_bad[rows[0], d - 1], s_bad[rows[1], 0] = -0.5, np.nan
    mu, z, ell = _dev(c["mu"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    cw, aw = _weights(ca, c, q, dt)
    tr, quad, none_bad = devp.psi2_rows_quad(mu, _dev(c["s"], dt), z, ell, SF, cw, aw)
    btr, bquad, bad = devp.psi2_rows_quad(mu, _dev(s_bad, dt), z, ell, SF, cw, aw)
    assert float(bad.item()) == 2.0 and float(none_bad.item()) == 0.0
    assert bool((btr[rows] == 0).all()) and bool((bquad[rows] == 0).all())
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert torch.equal(_bits(btr[keep]), _bits(tr[keep])) and torch.equal(_bits(bquad[keep]), _bits(quad[keep]))
    assert bool((tr[rows] != 0).all())                                         # the planted rows were live before


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rows_quad_footprint(ca, dt):
    """Inside guarded buffers, c, a and quad at wide pitches: the call writes tr, its n x q block of quad and bad[0] and
    nothing else; inputs, the weights with their padding and c's strict upper triangle (poisoned: never read) and the
    guards keep their bytes; what the scratch held does not matter (the three poisoned runs give the same bits)."""
    from cimrgp_amd import _lib
    n, m, d, q = 150, 70, 3, QMAX
    tdt, dtid = TDT[dt], (_lib.F64 if dt == "f64" else _lib.F32)
    c = _case(n, m, d, seed=3)
    lib = _lib.load()

    def const(name, a, t=tdt):
        a = np.ascontiguousarray(a).reshape(-1)
        return Guarded(name, a.size, t, CUDA).vec(CONST, a.size, values=a)

    mu, s, z, ell = const("mu", c["mu"]), const("s", c["s"]), const("z", c["z"]), const("ell", c["ell"], torch.float64)
    cm = Guarded("c", (m + 3) * wide_ld(m), tdt, CUDA, ld=wide_ld(m)).mark(CONST, m, m, part="lower", values=c["c"])
    am = Guarded("a", (m + 3) * wide_ld(q), tdt, CUDA, ld=wide_ld(q)).mark(CONST, m, q, values=c["a"])
    tr = Guarded("tr", n, tdt, CUDA).vec(OUT, n)
    quad = Guarded("quad", (n + 3) * wide_ld(q), tdt, CUDA, ld=wide_ld(q)).mark(OUT, n, q)
    nbytes = int(lib.cimrgp_psi2_rows_quad_scratch_bytes(dtid, n, m, d, q))
    scratch = Guarded("scratch", nbytes, torch.uint8, CUDA).vec(JUNK, nbytes)
    bad = Guarded("bad", 1, torch.float64, CUDA).vec(OUT, 1)

    def call():
        _lib.check(lib.cimrgp_psi2_rows_quad(dtid, mu.ptr(), s.ptr(), z.ptr(), n, m, d, ell.ptr(), SF, cm.ptr(), cm.ld, am.ptr(), am.ld, q,
                                             tr.ptr(), quad.ptr(), quad.ld, scratch.ptr(), nbytes, bad.ptr(),
                                             torch.cuda.current_stream().cuda_stream), "cimrgp_psi2_rows_quad")

    run_contract([mu, s, z, ell, cm, am, tr, quad, scratch, bad], call, torch.cuda.synchronize)
    assert _show("footprint rows_quad %s" % dt, _ratios(tr.data, quad.mat(n, q), c["ref"], UNIT[dt], q)) <= 1.0
    assert float(bad.data[0].item()) == 0.0
