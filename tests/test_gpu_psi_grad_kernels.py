"""GPU tests of the psi gradient kernels (include/cimrgp_psi_grad.h; DESIGN.md, "Gradients of the bound on uncertain
inputs"): cimrgp_psi1_grad and cimrgp_psi2_grad against the longdouble oracle of tests/psi_grad_numpy.py entry by entry at
bounds that count roundings (``psi_grad_numpy.grad_bound``), then the bad rows, repeatability, the buffer footprint (the
helper of tests/test_gpu_buffer_contract.py) and, at s = 0, the agreement with cimrgp_cov_pair_grad_ard on K_fu."""
import functools

import numpy as np
import pytest

import psi_grad_numpy as pg
import psi_numpy as po
from test_gpu_buffer_contract import CONST, CUDA, JUNK, OUT, Guarded, run_contract, wide_ld
from test_gpu_psi_kernels import ELLS, SF, SHAPES, SLICED, TDT, UNIT, _bits, _dev, _ell_dev, _f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
KEYS = ("dmu", "ds", "dz", "sums")


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _weights(n, m, seed):
    """Random signed g1 (n x m) and a random symmetric g2 (m x m), float32-representable."""
    rng = np.random.RandomState(seed)
    g2 = rng.randn(m, m)
    return _f32(rng.randn(n, m)), _f32(g2 + g2.T)


@functools.lru_cache(maxsize=None)
def _case(n, m, d, seed=0, drop=None):
    """The problem of a shape (the inputs of tests/test_gpu_psi_kernels.py) with its weights, the longdouble gradients and
    the bounds' weights, once.  ``drop``: rows left out of the reference (the planted bad rows)."""
    mu, s, z, _ = po.problem(n, m, d, 100 * n + m + seed, ell0=ELLS[0])
    mu, s, z = _f32(mu), _f32(s), _f32(z)
    ell = np.array(ELLS[:d])
    g1, g2 = _weights(n, m, 7 * n + m + seed)
    keep = np.ones(n, dtype=bool)
    if drop:
        keep[list(drop)] = False
    ref = {1: (pg.psi1_grad(mu[keep], s[keep], z, ell, SF, g1[keep], LD), pg.psi1_grad(mu[keep], s[keep], z, ell, SF, g1[keep], LD, bound=True)),
           2: (pg.psi2_grad(mu[keep], s[keep], z, ell, SF, g2, LD), pg.psi2_grad(mu[keep], s[keep], z, ell, SF, g2, LD, bound=True))}
    return dict(mu=mu, s=s, z=z, ell=ell, g1=g1, g2=g2, keep=keep, ref=ref)


def _host(outs):
    return {k: t.double().cpu().numpy() for k, t in zip(KEYS, outs)}


def _ratios(got, ref, u, rows=None):
    """{key: max |got - ref| / bound}, every entry finite (asserted); ``rows``: the rows of dmu and ds that are compared."""
    val, wts = ref
    out = {}
    for k in KEYS:
        g = got[k][rows] if rows is not None and k in ("dmu", "ds") else got[k]
        assert np.isfinite(g).all(), k
        out[k] = float(np.asarray(np.abs(np.asarray(g, dtype=LD) - val[k]) / pg.grad_bound(val[k], wts[k], u), dtype=np.float64).max())
    return out


def _show(what, ratios):
    print("%s: err/bound %s" % (what, "  ".join("%s %.3f" % (k, ratios[k]) for k in KEYS)))
    return max(ratios.values())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_psi_grad_kernels_match_the_longdouble_oracle(ca, dt, n, m, d):
    """Every entry of dmu, ds, dz and sums of both calls: |got - ref| <= grad_bound (tests/psi_grad_numpy.py has the
    counting); two calls give the same bits; no row is bad.  g2 is given with NaN above its diagonal: only k <= j is read."""
    from cimrgp_amd import device_psi as devp
    c, u = _case(n, m, d), UNIT[dt]
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    g1 = torch.full((n, ca.device.padded_ld(m)), float("nan"), dtype=TDT[dt], device="cuda")
    g1[:, :m] = _dev(c["g1"], dt)
    g2 = torch.full((m, ca.device.padded_ld(m)), float("nan"), dtype=TDT[dt], device="cuda")
    g2[:, :m] = torch.tril(_dev(c["g2"], dt)) + torch.triu(torch.full((m, m), float("nan"), dtype=TDT[dt], device="cuda"), 1)
    one, again = devp.psi1_grad(mu, s, z, ell, SF, g1), devp.psi1_grad(mu, s, z, ell, SF, g1)
    two, again2 = devp.psi2_grad(mu, s, z, ell, SF, g2), devp.psi2_grad(mu, s, z, ell, SF, g2)
    for a, b in zip(one + two, again + again2):
        assert torch.equal(_bits(a), _bits(b))
    assert float(two[4].item()) == 0.0
    r1 = _show("psi1_grad %s (%d, %d, %d)" % (dt, n, m, d), _ratios(_host(one), c["ref"][1], u))
    r2 = _show("psi2_grad %s (%d, %d, %d)" % (dt, n, m, d), _ratios(_host(two[:4]), c["ref"][2], u))
    assert r1 <= 1.0 and r2 <= 1.0
    if (n, m, d) == SLICED:
        esz = 8 if dt == "f64" else 4
        assert devp.psi2_grad_scratch_bytes(n, m, d, TDT[dt]) == pg.psi2_grad_scratch_bytes(esz, n, m, d)
        assert devp.psi1_grad_scratch_bytes(n, m, d, TDT[dt]) == pg.psi1_grad_scratch_bytes(esz, n, m, d)
        assert pg._slices_for(n, 1)[0] >= 3 and n % pg._slices_for(n, 1)[1] != 0


#: cimrgp_psi1_grad with slices longer than one 64-row chunk: m = 4096 gives 64 column blocks and so at most 32 slices, and
#: n = 2113 then 27 slices of 80 rows, a chunk of 64 and one of 16 (asserted below)
CHUNKED = (2113, 4096, 1)


@functools.lru_cache(maxsize=None)
def _chunked_case():
    """The problem at CHUNKED with g1 and the longdouble psi1_grad and its bounds' weights, once for both dtypes."""
    n, m, d = CHUNKED
    mu, s, z, _ = po.problem(n, m, d, 100 * n + m, ell0=ELLS[0])
    mu, s, z = _f32(mu), _f32(s), _f32(z)
    ell, g1 = np.array(ELLS[:d]), _f32(np.random.RandomState(7 * n + m).randn(n, m))
    return dict(mu=mu, s=s, z=z, ell=ell, g1=g1,
                ref=(pg.psi1_grad(mu, s, z, ell, SF, g1, LD), pg.psi1_grad(mu, s, z, ell, SF, g1, LD, bound=True)))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_psi1_grad_over_slices_of_several_chunks_matches_the_longdouble_oracle(ca, dt):
    """The bound of test_psi_grad_kernels_match_the_longdouble_oracle at the one cheap shape whose slices span two chunks."""
    from cimrgp_amd import device_psi as devp
    n, m, d = CHUNKED
    assert pg._slices_for(n, -(-m // 64)) == (27, 80)
    c = _chunked_case()
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    g1 = torch.full((n, ca.device.padded_ld(m)), float("nan"), dtype=TDT[dt], device="cuda")
    g1[:, :m] = _dev(c["g1"], dt)
    one, again = devp.psi1_grad(mu, s, z, ell, SF, g1), devp.psi1_grad(mu, s, z, ell, SF, g1)
    for a, b in zip(one, again):
        assert torch.equal(_bits(a), _bits(b))
    assert _show("psi1_grad %s (%d, %d, %d)" % (dt, n, m, d), _ratios(_host(one), c["ref"], UNIT[dt])) <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,d", [(300, 65, 3), (150, 40, 2)])
def test_bad_rows_are_counted_zeroed_and_add_nothing(ca, dt, n, m, d):
    """Two planted rows (a negative and a NaN variance): bad = 2, their rows of dmu and ds are zeros, and every other entry
    is that of the data without them, within the bound."""
    from cimrgp_amd import device_psi as devp
    rows = (n // 3, n - 2)
    c, u = _case(n, m, d, seed=7, drop=rows), UNIT[dt]
    s_bad = c["s"].copy()
    s_bad[rows[0], d - 1], s_bad[rows[1], 0] = -0.5, np.nan
    z, ell = _dev(c["z"], dt), _ell_dev(c["ell"])
    out = devp.psi2_grad(_dev(c["mu"], dt), _dev(s_bad, dt), z, ell, SF, _dev(c["g2"], dt))
    assert float(out[4].item()) == 2.0
    got = _host(out[:4])
    for k in ("dmu", "ds"):
        assert (got[k][list(rows)] == 0.0).all(), k
    assert _show("psi2_grad with two bad rows %s (%d, %d, %d)" % (dt, n, m, d), _ratios(got, c["ref"][2], u, rows=c["keep"])) <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_psi_grad_footprint(ca, dt):
    """Inside guarded buffers, the weights at a wide pitch: both calls write dmu, ds, dz, sums (and bad[0]) and nothing else;
    inputs, the weights with their padding and g2's strict upper triangle (poisoned: never read) and the guards keep their
    bytes; what the scratch held does not matter (the three poisoned runs give the same bits)."""
    from cimrgp_amd import _lib
    n, m, d = 150, 70, 3
    tdt, dtid = TDT[dt], (_lib.F64 if dt == "f64" else _lib.F32)
    c = _case(n, m, d, seed=3)
    lib = _lib.load()

    def const(name, a, t=tdt):
        a = np.ascontiguousarray(a).reshape(-1)
        return Guarded(name, a.size, t, CUDA).vec(CONST, a.size, values=a)

    mu, s, z, ell = const("mu", c["mu"]), const("s", c["s"]), const("z", c["z"]), const("ell", c["ell"], torch.float64)
    g1 = Guarded("g1", (n + 3) * wide_ld(m), tdt, CUDA, ld=wide_ld(m)).mark(CONST, n, m, values=c["g1"])
    g2 = Guarded("g2", (m + 3) * wide_ld(m), tdt, CUDA, ld=wide_ld(m)).mark(CONST, m, m, part="lower", values=c["g2"])
    outs = {}
    for which in (1, 2):
        outs[which] = [Guarded("dmu%d" % which, n * d, tdt, CUDA).vec(OUT, n * d), Guarded("ds%d" % which, n * d, tdt, CUDA).vec(OUT, n * d),
                       Guarded("dz%d" % which, m * d, tdt, CUDA).vec(OUT, m * d),
                       Guarded("sums%d" % which, d + 1, torch.float64, CUDA).vec(OUT, d + 1)]
    nb1, nb2 = int(lib.cimrgp_psi1_grad_scratch_bytes(dtid, n, m, d)), int(lib.cimrgp_psi2_grad_scratch_bytes(dtid, n, m, d))
    sc1 = Guarded("scratch1", nb1, torch.uint8, CUDA).vec(JUNK, nb1)
    sc2 = Guarded("scratch2", nb2, torch.uint8, CUDA).vec(JUNK, nb2)
    bad = Guarded("bad", 1, torch.float64, CUDA).vec(OUT, 1)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def call():
        a, b = outs[1], outs[2]
        _lib.check(lib.cimrgp_psi1_grad(dtid, mu.ptr(), s.ptr(), z.ptr(), n, m, d, ell.ptr(), SF, g1.ptr(), g1.ld, a[0].ptr(), a[1].ptr(),
                                        a[2].ptr(), a[3].ptr(), sc1.ptr(), nb1, stream()), "cimrgp_psi1_grad")
        _lib.check(lib.cimrgp_psi2_grad(dtid, mu.ptr(), s.ptr(), z.ptr(), n, m, d, ell.ptr(), SF, g2.ptr(), g2.ld, b[0].ptr(), b[1].ptr(),
                                        b[2].ptr(), b[3].ptr(), sc2.ptr(), nb2, bad.ptr(), stream()), "cimrgp_psi2_grad")

    run_contract([mu, s, z, ell, g1, g2, sc1, sc2, bad] + outs[1] + outs[2], call, torch.cuda.synchronize)
    u = UNIT[dt]
    for which in (1, 2):
        a = outs[which]
        got = dict(dmu=a[0].data.view(n, d), ds=a[1].data.view(n, d), dz=a[2].data.view(m, d), sums=a[3].data)
        got = {k: t.double().cpu().numpy() for k, t in got.items()}
        assert _show("footprint psi%d_grad %s" % (which, dt), _ratios(got, c["ref"][which], u)) <= 1.0
    assert float(bad.data[0].item()) == 0.0


def test_at_zero_variance_psi1_grad_is_the_pair_contraction_of_k_fu(ca):
    """s = 0: Psi1 = K_fu, so dz and the length-scale sums of cimrgp_psi1_grad equal what cimrgp_cov_pair_grad_ard gives for
    the same weights on the inputs scaled by 1 / l (dz back through 1 / l), within the sum of both bounds; the scaled
    operands carry two more roundings per difference, 5 d + 4 per unit of exponent in place of 3 d + 2, as the
    shared-variance composition's bound has it (tests/test_gpu_psi_kernels.py)."""
    from cimrgp_amd import device_psi as devp
    n, m, d, dt, u = 300, 65, 3, "f64", UNIT["f64"]
    c = _case(n, m, d, seed=11)
    zero = np.zeros_like(c["s"])
    mu, z, ell, g1 = _dev(c["mu"], dt), _dev(c["z"], dt), _ell_dev(c["ell"]), _dev(c["g1"], dt)
    _, _, dz, sums = devp.psi1_grad(mu, _dev(zero, dt), z, ell, SF, g1)
    scale = _dev(1.0 / c["ell"], dt)
    psums, db = ca.device.cov_pair_grad_ard((mu * scale).contiguous(), (z * scale).contiguous(), g1, 1.0, SF)
    val = pg.psi1_grad(c["mu"], zero, c["z"], c["ell"], SF, c["g1"], LD)
    w_own = pg.psi1_grad(c["mu"], zero, c["z"], c["ell"], SF, c["g1"], LD, bound=True)
    w_pair = pg.psi1_grad(c["mu"], zero, c["z"], c["ell"], SF, c["g1"], LD, bound=True, roundings=5 * d + 4)
    both = {k: pg.grad_bound(val[k], w_own[k], u) + pg.grad_bound(val[k], w_pair[k], u) for k in ("dz", "sums")}
    rz = float((np.abs(dz.cpu().numpy() - (db * scale).cpu().numpy()) / both["dz"]).max())
    rs = float((np.abs(sums.cpu().numpy() - psums.cpu().numpy()) / both["sums"]).max())
    ro = _show("psi1_grad at s = 0", _ratios(_host(devp.psi1_grad(mu, _dev(zero, dt), z, ell, SF, g1)), (val, w_own), u))
    print("s = 0 against cimrgp_cov_pair_grad_ard: dz diff/bounds %.3f, sums diff/bounds %.3f" % (rz, rs))
    assert rz <= 1.0 and rs <= 1.0 and ro <= 1.0
