"""GPU tests of the psi kernels (include/cimrgp_psi.h; DESIGN.md, "Sparse GP regression on uncertain inputs"): cimrgp_psi1
and cimrgp_psi2 against the longdouble oracle of tests/psi_numpy.py entry by entry at bounds that count roundings, then
repeatability, independence of a row from n, the count of bad rows, the buffer footprint (the helper of
tests/test_gpu_buffer_contract.py) and the agreement of the per-row kernels with the shared-variance composition."""
import functools

import numpy as np
import pytest

import psi_numpy as po
from test_gpu_buffer_contract import CONST, CUDA, JUNK, OUT, UNTOUCHED, Guarded, run_contract, wide_ld

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
#: (n, m, d): one of each; ragged tiles of 64; m one past a tile and d = 3; two tile rows and the largest d; and n = 150, which
#: the header's rule cuts into three slices of 64 rows, the last one ragged (asserted below); then the remaining instances of
#: d at (130, 70): two tile rows at edge 64 and three at edge 32 with a ragged last tile, three slices
SHAPES = [(1, 1, 1), (255, 63, 2), (300, 65, 3), (257, 130, 8), (150, 40, 2)] + [(130, 70, d) for d in (4, 5, 6, 7)]
SLICED = (150, 40, 2)
#: exactly representable in float32, so that both dtypes see the same problem and share one reference
SF = 1.375
ELLS = [0.75, 1.25, 1.0, 0.875, 1.5, 1.125, 0.625, 1.0]


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", TDT[dt]).contiguous()


def _f32(a):
    """Values both dtypes hold exactly."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(n, m, d, seed=0):
    """The problem of a shape (float32-representable inputs) and its longdouble reference with the bounds' weights, once."""
    mu, s, z, _ = po.problem(n, m, d, 100 * n + m + seed, ell0=ELLS[0])
    mu, s, z = _f32(mu), _f32(s), _f32(z)
    ell = np.array(ELLS[:d])
    return dict(mu=mu, s=s, z=z, ell=ell, psi1=po.psi1_terms(mu, s, z, ell, SF), psi2=po.psi2_terms(mu, s, z, ell, SF))


def _ell_dev(ell):
    return torch.as_tensor(np.asarray(ell, dtype=np.float64)).to("cuda")


def _nan_matrix(ca, rows, cols, dt):
    return torch.full((rows, ca.device.padded_ld(cols)), float("nan"), dtype=TDT[dt], device="cuda")


def _worst(got, ref, bound, where=None):
    """max |got - ref| / bound over ``where`` (all entries finite, asserted)."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - ref)
    ratio = np.asarray(err / bound, dtype=np.float64)
    if where is not None:
        got, ratio = got[where], ratio[where]
    assert np.isfinite(got).all(), "a non-finite entry"
    return float(ratio.max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_psi_kernels_match_the_longdouble_oracle(ca, dt, n, m, d):
    """Entry by entry: |Psi1 - ref| <= u Psi1 [(3 d + 2) t + 2 d + 12] + u Psi1 and |Psi2 - ref| <= u sum_i term [n + (3 d + 2)
    (t + delta) + 2 d + 12] + u Psi2 (tests/psi_numpy.py has the counting), each plus the format's underflow floor; the
    pair of inducing inputs 40 length-scales apart underflows to (about) 0 and is never NaN; two runs give the same bits;
    no row is bad.  Only the lower triangle of Psi2 is written (the buffer starts as NaN)."""
    from cimrgp_amd import device_psi as devp
    c, u, tdt = _case(n, m, d), UNIT[dt], TDT[dt]
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    out1 = devp.psi1(mu, s, z, ell, SF, out=_nan_matrix(ca, n, m, dt))
    out2, bad = devp.psi2(mu, s, z, ell, SF, out=_nan_matrix(ca, m, m, dt))
    again1 = devp.psi1(mu, s, z, ell, SF, out=_nan_matrix(ca, n, m, dt))
    again2, _ = devp.psi2(mu, s, z, ell, SF, out=_nan_matrix(ca, m, m, dt))
    assert float(bad.item()) == 0.0
    assert torch.equal(_bits(out1[:, :m]), _bits(again1[:, :m]))
    low = torch.tril(torch.ones((m, m), dtype=torch.bool, device="cuda"))
    assert torch.equal(_bits(out2[:m, :m][low]), _bits(again2[:m, :m][low]))
    assert bool(torch.isnan(out1[:, m:]).all()) and bool(torch.isnan(out2[:m, :m][~low]).all()) and bool(torch.isnan(out2[:m, m:]).all())
    p1, w1 = c["psi1"]
    p2, w2 = c["psi2"]
    r1 = _worst(out1[:n, :m].double().cpu().numpy(), p1, po.bound(p1, w1, u))
    il = np.tril_indices(m)
    got2 = out2[:m, :m].double().cpu().numpy()
    r2 = _worst(got2, p2, po.bound(p2, w2, u, n), il)
    print("psi %s (%d, %d, %d): psi1 err/bound %.3f, psi2 err/bound %.3f" % (dt, n, m, d, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0
    if m >= 2:
        assert 0.0 <= got2[m - 1, 0] <= 1e-30                    # 40 length-scales apart
    if (n, m, d) == SLICED:
        assert devp.psi2_slices(n, m) >= 3 and n % po.slices(n, m)[1] != 0
        assert devp.psi2_scratch_bytes(n, m, d, tdt) > devp.psi2_scratch_bytes(1, m, d, tdt)
        assert devp.psi2_scratch_bytes(n, m, d, tdt) == po.scratch_bytes(8 if dt == "f64" else 4, n, m, d)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_row_of_psi1_does_not_depend_on_n_or_its_place(ca, dt):
    from cimrgp_amd import device_psi as devp
    n, m, d = 300, 65, 3
    c = _case(n, m, d)
    mu, s, z, ell = _dev(c["mu"], dt), _dev(c["s"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    whole = devp.psi1(mu, s, z, ell, SF)
    for a, b in ((0, 1), (100, 111), (297, 300)):
        part = devp.psi1(mu[a:b].contiguous(), s[a:b].contiguous(), z, ell, SF)
        assert torch.equal(_bits(part[:b - a, :m]), _bits(whole[a:b, :m])), (a, b)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [60, 300])
def test_bad_rows_are_counted_and_add_nothing(ca, dt, n):
    """Two planted rows (a negative and a NaN variance): bad = 2 and Psi2 is that of the data without them -- to the bit in
    one slice (n = 60: a thread adds its rows in order, and an exact 0 changes no sum), within the bound otherwise."""
    from cimrgp_amd import device_psi as devp
    m, d, u = 65, 3, UNIT[dt]
    c = _case(n, m, d, seed=7)
    keep = np.ones(n, dtype=bool)
    keep[[n // 3, n - 2]] = False
    s_bad = c["s"].copy()
    s_bad[n // 3, 1], s_bad[n - 2, 0] = -0.5, np.nan
    z, ell = _dev(c["z"], dt), _ell_dev(c["ell"])
    got, bad = devp.psi2(_dev(c["mu"], dt), _dev(s_bad, dt), z, ell, SF)
    clean, none_bad = devp.psi2(_dev(c["mu"][keep], dt), _dev(c["s"][keep], dt), z, ell, SF)
    assert float(bad.item()) == 2.0 and float(none_bad.item()) == 0.0
    low = torch.tril(torch.ones((m, m), dtype=torch.bool, device="cuda"))
    assert bool(torch.isfinite(got[:m, :m][low]).all())
    if devp.psi2_slices(n, m) == 1:
        assert torch.equal(_bits(got[:m, :m][low]), _bits(clean[:m, :m][low]))
    else:
        p2, w2 = po.psi2_terms(c["mu"][keep], c["s"][keep], c["z"], c["ell"], SF)
        il = np.tril_indices(m)
        ratio = _worst(got[:m, :m].double().cpu().numpy(), p2, po.bound(p2, w2, u, n), il)
        print("psi2 with two bad rows %s n=%d: err/bound %.3f" % (dt, n, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_psi_footprint(ca, dt):
    """Inside guarded buffers at a wide pitch: Psi1 writes its n x m block, Psi2 the lower triangle of its m x m block and
    bad[0]; inputs, padding, the strict upper triangle and the guards keep their bytes; what the scratch held does not
    matter (the three poisoned runs give the same bits)."""
    from cimrgp_amd import _lib
    n, m, d = 150, 70, 3
    tdt, dtid = TDT[dt], (_lib.F64 if dt == "f64" else _lib.F32)
    c = _case(n, m, d, seed=3)
    lib = _lib.load()

    def const(name, a, t=tdt):
        a = np.ascontiguousarray(a).reshape(-1)
        return Guarded(name, a.size, t, CUDA).vec(CONST, a.size, values=a)

    mu, s, z, ell = const("mu", c["mu"]), const("s", c["s"]), const("z", c["z"]), const("ell", c["ell"], torch.float64)
    out1 = Guarded("Psi1", (n + 3) * wide_ld(m), tdt, CUDA, ld=wide_ld(m)).mark(OUT, n, m)
    out2 = Guarded("Psi2", (m + 3) * wide_ld(m), tdt, CUDA, ld=wide_ld(m)).mark(OUT, m, m, part="lower")
    assert int((out2.role == UNTOUCHED).sum()) > m * (m - 1) // 2
    nbytes = int(lib.cimrgp_psi2_scratch_bytes(dtid, n, m, d))
    scratch = Guarded("scratch", nbytes, torch.uint8, CUDA).vec(JUNK, nbytes)
    bad = Guarded("bad", 1, torch.float64, CUDA).vec(OUT, 1)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(lib.cimrgp_psi1(dtid, mu.ptr(), s.ptr(), z.ptr(), n, m, d, ell.ptr(), SF, out1.ptr(), out1.ld, stream()), "cimrgp_psi1")
        _lib.check(lib.cimrgp_psi2(dtid, mu.ptr(), s.ptr(), z.ptr(), n, m, d, ell.ptr(), SF, out2.ptr(), out2.ld, scratch.ptr(), nbytes,
                                   bad.ptr(), stream()), "cimrgp_psi2")

    run_contract([mu, s, z, ell, out1, out2, scratch, bad], call, torch.cuda.synchronize)
    u = UNIT[dt]
    p1, w1 = c["psi1"]
    p2, w2 = c["psi2"]
    assert _worst(out1.mat(n, m).double().cpu().numpy(), p1, po.bound(p1, w1, u)) <= 1.0
    assert _worst(out2.mat(m, m).double().cpu().numpy(), p2, po.bound(p2, w2, u, n), np.tril_indices(m)) <= 1.0
    assert float(bad.data[0].item()) == 0.0


@pytest.mark.parametrize("svec", [(0.3, 0.0, 2.5), (0.0, 0.0, 0.0)])
def test_the_two_routes_agree(ca, svec):
    """One variance vector repeated over the rows: cimrgp_psi2 equals the shared-variance composition (two scalings,
    cimrgp_cov_cross, cimrgp_wsyrk_tn and the m x m factor C) within the sum of both bounds.  The composition's exponent
    is the same positive sum t + delta, split over G_ij, G_ik and C_jk; its operands are scaled first (two more roundings
    per difference): 5 d + 4 roundings per unit of exponent in place of 3 d + 2.  At s = 0 the composition is cimrgp_cov_cross
    and cimrgp_wsyrk_tn of it as they stand: Psi1 = K_fu and Psi2 = K_uf K_fu within the same bounds."""
    from cimrgp_amd import UncertainInputBlock, device_psi as devp
    from cimrgp_amd.KernelClass import RBFKernel
    n, m, d, dt, u = 300, 65, 3, "f64", UNIT["f64"]
    c = _case(n, m, d, seed=11)
    sv = np.array(svec)
    s_rows = np.broadcast_to(sv, (n, d)).copy()
    mu, z, ell = _dev(c["mu"], dt), _dev(c["z"], dt), _ell_dev(c["ell"])
    got1 = devp.psi1(mu, _dev(s_rows, dt), z, ell, SF)
    got2, bad = devp.psi2(mu, _dev(s_rows, dt), z, ell, SF)
    blk = UncertainInputBlock(mu, sv, z, RBFKernel(l=1.0, sf=SF, noise=0.5), lengthscales=c["ell"])
    sh1 = blk._psi1(mu, blk.x_var)
    sh2, _ = blk._psi2()
    if not sv.any():
        sh1 = ca.device.rbf_cross(blk._xs, blk._zs, 1.0, SF)
        sh2 = ca.device.wsyrk_tn(sh1, n, m, torch.ones(n, dtype=torch.float64, device="cuda"))[0]
    p1, w1 = po.psi1_terms(c["mu"], s_rows, c["z"], c["ell"], SF)
    p2, w2 = po.psi2_terms(c["mu"], s_rows, c["z"], c["ell"], SF)
    _, w1s = po.psi1_terms(c["mu"], s_rows, c["z"], c["ell"], SF, roundings=5 * d + 4)
    _, w2s = po.psi2_terms(c["mu"], s_rows, c["z"], c["ell"], SF, roundings=5 * d + 4)
    il = np.tril_indices(m)
    both1 = po.bound(p1, w1, u) + po.bound(p1, w1s, u)
    both2 = po.bound(p2, w2, u, n) + po.bound(p2, w2s, u, n)
    r1 = float((np.abs(got1[:n, :m].cpu().numpy() - sh1[:n, :m].cpu().numpy()) / both1).max())
    r2 = float((np.abs(got2[:m, :m].cpu().numpy() - sh2[:m, :m].cpu().numpy()) / both2)[il].max())
    o2 = _worst(sh2[:m, :m].cpu().numpy(), p2, po.bound(p2, w2s, u, n), il)
    print("two routes s=%s: psi1 diff/bounds %.3f, psi2 diff/bounds %.3f, shared route err/bound %.3f" % (svec, r1, r2, o2))
    assert float(bad.item()) == 0.0 and r1 <= 1.0 and r2 <= 1.0 and o2 <= 1.0
