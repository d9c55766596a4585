"""GPU tests of the dense covariance kernels (gram.hip, misc.hip, common.hpp's Cov<COV>) against the longdouble oracle of
tests/cov_numpy.py, entry by entry at bounds that count roundings: cimrgp_cov_gram (the 64 x 64 tiles and the wide lower
tiles), cimrgp_cov_cross, the fused mean cimrgp_cov_predict_mean, the gradient contraction cimrgp_cov_lml_grad[_ard] and
the two small reductions on block_sum; then every layout the C ABI admits -- a pitch equal to an odd number of columns,
one more than that, and a base one element off a 16-byte boundary -- for the kernels with an aligned and an element arm
(bit-identical results, guards untouched) and for the other entries that take any pitch >= cols.

Every buffer a kernel writes or reads at a pitch is a :class:`Placed` matrix: NaN in front, behind and in the padding."""
import functools

import numpy as np
import pytest

import cov_numpy as cn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
NPT = {"f64": np.float64, "f32": np.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
DTS = ["f64", "f32"]
#: exactly representable in float32
SF2, DIAG_ADD, NOISE = 1.375, 0.05, 0.05
ELLS = (0.6, 2.0 ** -4, 16.0)
GRAM_N = (1, 63, 64, 65, 127, 128, 129, 191, 193, 320)
CROSS_SHAPES = ((1, 1), (65, 130), (193, 67))
NMAX = 320
#: where the cross-Gram's columns start in the shared problem: K[:na, CROSS_COL0:CROSS_COL0 + nb] is not symmetric
CROSS_COL0 = 40
GUARD = 64
#: power-of-two length-scales: x / ell is exact in both dtypes
ARD_ELLS = np.array([0.5, 2.0, 1.0, 0.25, 4.0, 1.0, 0.5, 2.0])
LAYOUTS = ("padded", "tight", "plus1", "shifted")


@pytest.fixture(scope="module")
def ca():
    import cimrgp_amd
    cimrgp_amd.device.require_gpu()
    return cimrgp_amd


def _lib():
    from cimrgp_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.check(getattr(L.load(), name)(*args), name)


def _dt(dt):
    return _lib().F64 if dt == "f64" else _lib().F32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda", TDT[dt]).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _padded_ld(n):
    from cimrgp_amd import device
    return device.padded_ld(n)


class Placed(object):
    """A rows x cols matrix of pitch ld inside a NaN-filled allocation: GUARD elements in front (+ one more for the
    "shifted" layout, which moves the base off every 16-byte boundary), the padding columns, GUARD elements behind.
    ``values`` (rows x cols) fills the matrix (an input); otherwise it stays NaN (an output)."""

    def __init__(self, rows, cols, layout, dt, values=None):
        assert layout in LAYOUTS
        if layout == "tight":
            assert cols % 2 == 1, "the tight layout is for an odd number of columns"
        self.rows, self.cols, self.layout = rows, cols, layout
        self.ld = {"padded": _padded_ld(cols), "tight": cols, "plus1": cols + 1, "shifted": _padded_ld(cols)}[layout]
        self.off = GUARD + (1 if layout == "shifted" else 0)
        self.full = torch.full((self.off + rows * self.ld + GUARD,), float("nan"), dtype=TDT[dt], device="cuda")
        assert self.full.data_ptr() % 16 == 0
        self.inside = torch.zeros(self.full.numel(), dtype=torch.bool, device="cuda")
        self.inside[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, :cols] = True
        if values is not None:
            self.mat().copy_(values if isinstance(values, torch.Tensor) else _dev(values, dt))

    def ptr(self):
        return self.full.data_ptr() + self.off * self.full.element_size()

    def mat(self):
        return self.full[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def outside_is_nan(self):
        return bool(torch.isnan(self.full[~self.inside]).all())


def _guarded(count, tdt, values=None):
    """(allocation, view): ``count`` contiguous elements between two NaN guards; ``values`` fills them, else they are NaN."""
    full = torch.full((2 * GUARD + count,), float("nan"), dtype=tdt, device="cuda")
    view = full[GUARD:GUARD + count]
    if values is not None:
        view.copy_(values.reshape(-1))
    return full, view


def _guards_are_nan(full, count):
    return bool(torch.isnan(full[:GUARD]).all()) and bool(torch.isnan(full[GUARD + count:]).all())


def _worst(got, ref, bnd, where=None):
    """max |got - ref| / bound over ``where`` (those entries finite, asserted)."""
    got = np.asarray(got, dtype=np.float64)
    ratio = np.asarray(np.abs(np.asarray(got, dtype=cn.LD) - ref) / bnd, dtype=np.float64)
    if where is not None:
        got, ratio = got[where], ratio[where]
    assert np.isfinite(got).all(), "a non-finite entry"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ Gram and cross-Gram ----
@functools.lru_cache(maxsize=None)
def _gram_case(d, ell, cov, offset):
    """The shared problem of NMAX points (a case of n points takes the first n: the planted rows come first) and its
    longdouble Gram matrix with the bound's weights, once for both dtypes, every n and both entries."""
    x = cn.problem(NMAX, d, 11 + d, offset)
    k, w = cn.value_terms(x, x, cov, ell, SF2)
    return x, k, w


def _gram_checks(dt, cov, d, offset):
    u, npt = UNIT[dt], NPT[dt]
    worst = 0.0
    for ell in ELLS:
        x, k, w = _gram_case(d, ell, cov, offset)
        xd = _dev(x, dt)
        for n in GRAM_N:
            ref = k[:n, :n] + DIAG_ADD * np.eye(n)
            bnd = cn.bound(ref, w[:n, :n], u)
            for lower_only in (0, 1):
                outs = []
                for _ in range(2):
                    out = Placed(n, n, "padded", dt)
                    _call("cimrgp_cov_gram", _dt(dt), cov, xd.data_ptr(), n, d, ell, SF2, DIAG_ADD, out.ptr(), out.ld, lower_only, _stream())
                    outs.append(out)
                where = np.tril_indices(n) if lower_only else None
                low = torch.tril(torch.ones((n, n), dtype=torch.bool, device="cuda"))
                a, b = outs[0].mat(), outs[1].mat()
                assert torch.equal(_bits(a[low]), _bits(b[low])) and (lower_only or torch.equal(_bits(a), _bits(b)))
                assert outs[0].outside_is_nan(), (n, ell, lower_only)
                got = _host(a)
                worst = max(worst, _worst(got, ref, bnd, where))
                assert got[0, 0] == float(npt(SF2) + npt(DIAG_ADD))
                if n > 1:
                    assert got[1, 0] == SF2                              # the coincident pair: exp(0) = 1, exactly
                if n > 3 and cov == 0 and ell <= 0.6:
                    assert 0.0 <= got[3, 0] < 1e-30 * SF2                # the far pair
    return worst


@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", DTS)
def test_gram_entries_are_inside_their_bounds(ca, dt, cov, d):
    """cimrgp_cov_gram, lower_only 0 (64 x 64 tiles) and 1 (k_gram_lower_wide), ell in {0.6, 2^-4, 16}, n over odd and even
    counts of tile rows and the wide tile's ragged last chunk: every entry (the lower triangle with lower_only) within
    u w + u k + 3 tiny, finite, the planted pairs exact, padding and guards NaN, two runs the same bits."""
    worst = _gram_checks(dt, cov, d, 0.0)
    print("cov_gram %s cov %d d %d: worst err/bound %.3f" % (dt, cov, d, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", DTS)
def test_gram_entries_beside_1024(ca, dt, cov, d):
    """The same with every coordinate moved by 1024: the differences are small beside the coordinates."""
    worst = _gram_checks(dt, cov, d, 1024.0)
    print("cov_gram at offset 1024 %s cov %d d %d: worst err/bound %.3f" % (dt, cov, d, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", DTS)
def test_cross_entries_are_inside_their_bounds(ca, dt, cov):
    """cimrgp_cov_cross at (na, nb) in {(1, 1), (65, 130), (193, 67)}: rows from the start of the shared problem, columns
    from its row 40, so the block is not symmetric."""
    u, worst = UNIT[dt], 0.0
    for d, offset in ((1, 0.0), (2, 0.0), (3, 0.0), (8, 0.0), (1, 1024.0), (3, 1024.0)):
        for ell in ELLS:
            x, k, w = _gram_case(d, ell, cov, offset)
            xd = _dev(x, dt)
            for na, nb in CROSS_SHAPES:
                cols = slice(CROSS_COL0, CROSS_COL0 + nb)
                ref, bnd = k[:na, cols], cn.bound(k[:na, cols], w[:na, cols], u)
                outs = []
                for _ in range(2):
                    out = Placed(na, nb, "padded", dt)
                    _call("cimrgp_cov_cross", _dt(dt), cov, xd.data_ptr(), na, xd[CROSS_COL0:].data_ptr(), nb, d, ell, SF2, out.ptr(),
                          out.ld, _stream())
                    outs.append(out)
                assert torch.equal(_bits(outs[0].mat()), _bits(outs[1].mat())) and outs[0].outside_is_nan()
                worst = max(worst, _worst(_host(outs[0].mat()), ref, bnd))
    print("cov_cross %s cov %d: worst err/bound %.3f" % (dt, cov, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ layouts ----
def _same_bits_everywhere(results, what):
    for layout, r in results[1:]:
        for a, b in zip(results[0][1], r):
            assert torch.equal(_bits(a), _bits(b)), "%s: layout %s differs from %s" % (what, layout, results[0][0])


@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("dt", DTS)
def test_gram_and_cross_layouts(ca, dt, cov):
    """gram_lanes' two store arms (the 16-byte non-temporal store; element stores where the chunk is not aligned or
    straddles column nb): the four layouts give the same bits and leave guards and padding alone."""
    d, ell, n, na, nb = 3, 0.6, 131, 70, 67
    x, k, w = _gram_case(d, ell, cov, 0.0)
    xd = _dev(x, dt)
    low = torch.tril(torch.ones((n, n), dtype=torch.bool, device="cuda"))
    for lower_only in (0, 1):
        res = []
        for layout in LAYOUTS:
            out = Placed(n, n, layout, dt)
            _call("cimrgp_cov_gram", _dt(dt), cov, xd.data_ptr(), n, d, ell, SF2, DIAG_ADD, out.ptr(), out.ld, lower_only, _stream())
            assert out.outside_is_nan(), (layout, lower_only)
            res.append((layout, [out.mat()[low] if lower_only else out.mat()]))
        _same_bits_everywhere(res, "cov_gram lower_only=%d" % lower_only)
        if not lower_only:
            ref = k[:n, :n] + DIAG_ADD * np.eye(n)
            assert _worst(_host(res[1][1][0]), ref, cn.bound(ref, w[:n, :n], UNIT[dt])) <= 1.0
    res = []
    for layout in LAYOUTS:
        out = Placed(na, nb, layout, dt)
        _call("cimrgp_cov_cross", _dt(dt), cov, xd.data_ptr(), na, xd[CROSS_COL0:].data_ptr(), nb, d, ell, SF2, out.ptr(), out.ld, _stream())
        assert out.outside_is_nan(), layout
        res.append((layout, [out.mat()]))
    _same_bits_everywhere(res, "cov_cross")
    cols = slice(CROSS_COL0, CROSS_COL0 + nb)
    assert _worst(_host(res[1][1][0]), k[:na, cols], cn.bound(k[:na, cols], w[:na, cols], UNIT[dt])) <= 1.0


@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("dt", DTS)
def test_cross_grad_layouts(ca, dt, cov):
    """cimrgp_cov_cross_grad's d + 1 output slabs (one matrix of (d + 1) na rows: slab stride na x pitch): the 16-byte store
    and the element stores give the same bits; slab 0 is cimrgp_cov_cross's output."""
    d, ell, na, nb = 3, 0.6, 70, 67
    x, k, w = _gram_case(d, ell, cov, 0.0)
    xd = _dev(x, dt)
    res = []
    for layout in LAYOUTS:
        out = Placed((d + 1) * na, nb, layout, dt)
        _call("cimrgp_cov_cross_grad", _dt(dt), cov, xd.data_ptr(), na, xd[CROSS_COL0:].data_ptr(), nb, d, ell, SF2, out.ptr(), out.ld,
              na * out.ld, _stream())
        assert out.outside_is_nan(), layout
        assert bool(torch.isfinite(out.mat()).all())
        res.append((layout, [out.mat()]))
    _same_bits_everywhere(res, "cov_cross_grad")
    cross = Placed(na, nb, "tight", dt)
    _call("cimrgp_cov_cross", _dt(dt), cov, xd.data_ptr(), na, xd[CROSS_COL0:].data_ptr(), nb, d, ell, SF2, cross.ptr(), cross.ld, _stream())
    assert torch.equal(_bits(res[1][1][0][:na]), _bits(cross.mat()))


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("dt", DTS)
def test_pair_grad_layouts(ca, dt, cov, ard):
    """cimrgp_cov_pair_grad[_ard] reads G with one 16-byte load per lane, or element by element where the chunk is not
    aligned or straddles column nb: the sums and db have the same bits for the four layouts of G, and the NaN around G
    reaches neither."""
    d, ell, na, nb = 3, 0.6, 70, 67
    x = _gram_case(d, ell, cov, 0.0)[0]
    xd = _dev(x, dt)
    g = _f32(np.random.RandomState(5).randn(na, nb))
    L = _lib().load()
    name = "cimrgp_cov_pair_grad_ard" if ard else "cimrgp_cov_pair_grad"
    nbytes = int(getattr(L, name + "_scratch_bytes")(na, nb, d))
    nsums = 1 + d if ard else 2
    res = []
    for layout in LAYOUTS:
        gp = Placed(na, nb, layout, dt, values=g)
        scratch = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
        sums = torch.full((nsums,), float("nan"), dtype=torch.float64, device="cuda")
        db = torch.full((nb, d), float("nan"), dtype=TDT[dt], device="cuda")
        _call(name, _dt(dt), cov, xd.data_ptr(), na, xd[CROSS_COL0:].data_ptr(), nb, d, gp.ptr(), gp.ld, ell, SF2, 1.0, 0, sums.data_ptr(),
              db.data_ptr(), scratch.data_ptr(), nbytes, _stream())
        assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(db).all()), layout
        assert gp.outside_is_nan()
        res.append((layout, [sums, db]))
    _same_bits_everywhere(res, name)
    # sums[0] = sum G k, k in the dtype and the sum in FP64: the entries' own bounds weighted by |G|, + the FP64 sum's steps
    kref, wref = cn.value_terms(x[:na], x[CROSS_COL0:CROSS_COL0 + nb], cov, ell, SF2)
    bnd = float((np.abs(g) * cn.bound(kref, wref, UNIT[dt])).sum() + 2.0 ** -53 * (na + 64) * (np.abs(g) * kref).sum())
    assert abs(float(res[0][1][0][0]) - float((g * kref).sum())) <= bnd


# the other entries that admit any pitch >= cols read their operand element by element (solve.hip: k_fwd_update,
# k_bwd_update, k_predict_from_w; sparse.hip: k_sparse_rowsq, k_sparse_tail; sparse_post.hip: k_sparse_tail_grad,
# k_sparse_loo; misc.hip: k_logdet_half, k_add_diag): one odd pitch each, bit-equal to the padded pitch
ODD_PITCH = ("padded", "tight")          # the padded pitch, and pitch = cols with cols odd (Placed asserts that)


@pytest.mark.parametrize("dt", DTS)
def test_solves_at_an_odd_pitch(ca, dt):
    """cimrgp_potrs and cimrgp_solve_lt with the factor at ldl = n (odd): the bits of the padded pitch."""
    from test_gpu_buffer_contract import _factored
    n, q = 301, 3
    rng, lower, wsv = _factored(ca.device, n, TDT[dt], 77)
    nan = torch.full_like(lower, float("nan"))
    lower = torch.where(torch.tril(torch.ones_like(lower, dtype=torch.bool)), lower, nan)
    rhs = _f32(rng.normal(size=(n, q)))
    res = []
    for layout in ODD_PITCH:
        lp = Placed(n, n, layout, dt, values=lower)
        r, z = _dev(rhs, dt), torch.full((n, q), float("nan"), dtype=TDT[dt], device="cuda")
        scratch = torch.full((2 * q * n,), float("nan"), dtype=TDT[dt], device="cuda")
        _call("cimrgp_potrs", _dt(dt), lp.ptr(), n, lp.ld, wsv.data_ptr(), r.data_ptr(), q, z.data_ptr(), scratch.data_ptr(), _stream())
        z2 = z.clone()
        _call("cimrgp_solve_lt", _dt(dt), lp.ptr(), n, lp.ld, wsv.data_ptr(), z2.data_ptr(), q, scratch.data_ptr(), _stream())
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(z).all())
        res.append((layout, [r, z, z2]))
    _same_bits_everywhere(res, "potrs / solve_lt")
    assert torch.equal(_bits(res[0][1][0]), _bits(res[0][1][2]))           # solve_lt of z is potrs' second half


@pytest.mark.parametrize("dt", DTS)
def test_predict_from_w_at_an_odd_pitch(ca, dt):
    ns, n, q = 5, 301, 3
    rng = np.random.RandomState(3)
    w, z, bias = _f32(0.05 * rng.randn(ns, n)), _dev(_f32(rng.randn(n, q)), dt), _dev([0.25, -1.5, 3.0], dt)
    res = []
    for layout in ODD_PITCH:
        wp = Placed(ns, n, layout, dt, values=w)
        mean = torch.full((ns, q), float("nan"), dtype=TDT[dt], device="cuda")
        var = torch.full((ns,), float("nan"), dtype=TDT[dt], device="cuda")
        _call("cimrgp_predict_from_w", _dt(dt), wp.ptr(), ns, n, wp.ld, z.data_ptr(), q, SF2, 0.5, None, bias.data_ptr(), mean.data_ptr(),
              var.data_ptr(), 0, _stream())
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())
        res.append((layout, [mean, var]))
    _same_bits_everywhere(res, "predict_from_w")


@pytest.mark.parametrize("dt", DTS)
def test_sparse_rows_at_an_odd_pitch(ca, dt):
    """cimrgp_sparse_lambda, _tail, _tail_grad and _loo: a wave per row, lane l reads columns l, l + 64, .. one by one."""
    n, m, d, q = 37, 131, 2, 3
    rng = np.random.RandomState(9)
    a, v = _f32(0.05 * rng.randn((d + 1) * n, m)), _f32(0.05 * rng.randn((d + 1) * n, m))
    gamma, r = _dev(_f32(rng.randn(m, q)), dt), _dev(_f32(rng.randn(n, q)), dt)
    tdt = TDT[dt]
    new = lambda *shape, t=tdt: torch.full(shape, float("nan"), dtype=t, device="cuda")
    res = []
    for layout in ODD_PITCH:
        ap, vp = Placed((d + 1) * n, m, layout, dt, values=a), Placed((d + 1) * n, m, layout, dt, values=v)
        lam, w, sums = new(n), new(n), new(3, t=torch.float64)
        _call("cimrgp_sparse_lambda", _dt(dt), ap.ptr(), n, m, ap.ld, SF2, NOISE, 0, lam.data_ptr(), w.data_ptr(), sums.data_ptr(), _stream())
        mean, var = new(n, q), new(n)
        _call("cimrgp_sparse_tail", _dt(dt), ap.ptr(), vp.ptr(), n, m, ap.ld, gamma.data_ptr(), q, SF2, 0.0, mean.data_ptr(), var.data_ptr(),
              0, _stream())
        mg, vg = new(n, d, q), new(n, d)
        _call("cimrgp_sparse_tail_grad", _dt(dt), ap.ptr(), vp.ptr(), n, m, d, ap.ld, n * ap.ld, gamma.data_ptr(), q, mg.data_ptr(),
              vg.data_ptr(), 0, _stream())
        lm, lv, bad = new(n, q), new(n), torch.zeros(1, dtype=torch.int32, device="cuda")
        _call("cimrgp_sparse_loo", _dt(dt), ap.ptr(), vp.ptr(), n, m, ap.ld, gamma.data_ptr(), r.data_ptr(), q, SF2, NOISE, 0, lm.data_ptr(),
              lv.data_ptr(), bad.data_ptr(), _stream())
        outs = [lam, w, sums, mean, var, mg, vg, lm, lv]
        assert all(bool(torch.isfinite(o).all()) for o in outs) and int(bad.item()) == 0
        assert ap.outside_is_nan() and vp.outside_is_nan()
        res.append((layout, outs))
    _same_bits_everywhere(res, "sparse rows")


# --------------------------------------------------------------------------------------------------------- fused mean ----
def _alpha(n, q, seed):
    """Alternating signs down the rows: the sums cancel."""
    rng = np.random.RandomState(seed)
    return _f32(rng.uniform(0.5, 1.5, size=(n, q)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None])


@functools.lru_cache(maxsize=None)
def _mean_case(cov, d, q, n, ns, with_bias, accumulate):
    x = cn.problem(n, d, 5 * n + d, 0.0)
    xs = cn.problem(ns, d, 7 * ns + d, 0.0)
    xs[0] = x[0]                                                         # one test point on a training point
    alpha = _alpha(n, q, n + q)
    bias = _f32(np.linspace(-1.5, 3.0, q)) if with_bias else None
    pre = _f32(np.random.RandomState(ns + q).randn(ns, q)) if accumulate else None
    return x, xs, alpha, bias, pre, cn.mean_terms(x, alpha, xs, cov, 0.6, SF2, bias, pre)


@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", DTS)
def test_fused_mean_is_inside_its_bound(ca, dt, cov):
    """cimrgp_cov_predict_mean for d in {1, 3}, q in {1, 3, 8}, n one lane's worth, one short of and one past 32, and many
    sweeps; with and without bias; accumulating onto a prefilled output (one more rounding)."""
    u, worst = UNIT[dt], 0.0
    for d in (1, 3):
        for q in (1, 3, 8):
            for n, ns in ((1, 1), (31, 9), (33, 8), (700, 37)):
                for with_bias in (False, True):
                    for acc in (0, 1):
                        x, xs, alpha, bias, pre, (m, w) = _mean_case(cov, d, q, n, ns, with_bias, acc)
                        xd, xsd, ad = _dev(x, dt), _dev(xs, dt), _dev(alpha, dt)
                        bd = _dev(bias, dt) if with_bias else None
                        outs = []
                        for _ in range(2):
                            full, out = _guarded(ns * q, TDT[dt], _dev(pre, dt) if acc else None)
                            _call("cimrgp_cov_predict_mean", _dt(dt), cov, xd.data_ptr(), n, d, ad.data_ptr(), q, xsd.data_ptr(), ns, 0.6,
                                  SF2, bd.data_ptr() if with_bias else None, out.data_ptr(), acc, _stream())
                            assert _guards_are_nan(full, ns * q)
                            outs.append(out.clone())
                        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
                        got = _host(outs[0]).reshape(ns, q)
                        worst = max(worst, _worst(got, m, cn.bound(np.abs(m), w, u)))
    print("cov_predict_mean %s cov %d: worst err/bound %.3f" % (dt, cov, worst))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------- gradient contraction ----
GRAD_SHAPES = ((1, 1, 1), (64, 1, 2), (65, 2, 3), (129, 3, 8), (300, 8, 5))
#: 47 tile rows, 1128 records: the final kernel's 1024 threads take a second trip
GRAD_BIG = (2945, 2, 8)


@functools.lru_cache(maxsize=None)
def _grad_case(n, d, q, cov, ard, wide):
    """x (the planted rows included), a random symmetric ``Kinv`` (the kernel is a contraction: no inverse is needed) and
    alpha, all float32-representable, and the longdouble gradient with its weights.  ``wide``: length-scales of 16 (ARD: 8
    times the vector), at which every tile carries weight -- the setting of the mutants in tests/test_cov_host.py."""
    rng = np.random.RandomState(1000 * n + 10 * d + q)
    x = cn.problem(n, d, n + d, 0.0)
    k = rng.randn(n, n)
    kinv = _f32((k + k.T) / 2)
    alpha = _alpha(n, q, n + q)
    ell = _grad_ell(d, ard, wide)
    upper_nan = kinv.copy()
    upper_nan[np.triu_indices(n, 1)] = np.nan
    return x, upper_nan, alpha, cn.lml_grad_terms(x, upper_nan, alpha, q, cov, ell, SF2, NOISE, ard)


def _grad_ell(d, ard, wide):
    return ARD_ELLS[:d] * (8.0 if wide else 1.0) if ard else (16.0 if wide else 0.6)


def _run_grad(dt, cov, n, d, q, ard, wide=False):
    x, kinv, alpha, (g, w, s) = _grad_case(n, d, q, cov, ard, wide)
    ell = _grad_ell(d, ard, wide)
    xin = x / ell if ard else x
    xd, ad = _dev(xin, dt), _dev(alpha, dt)
    kp = Placed(n, n, "padded", dt, values=kinv)                          # NaN strictly above the diagonal and all around
    nbytes = int(_lib().load().cimrgp_lml_grad_scratch_bytes(n))
    nout = d + 2 if ard else 3
    outs = []
    for poison in (float("nan"), 1e300):
        scratch = torch.full((nbytes // 8,), poison, dtype=torch.float64, device="cuda")
        full, out = _guarded(nout, torch.float64)
        if ard:
            _call("cimrgp_cov_lml_grad_ard", _dt(dt), cov, xd.data_ptr(), n, d, kp.ptr(), kp.ld, ad.data_ptr(), q, SF2, NOISE,
                  out.data_ptr(), scratch.data_ptr(), _stream())
        else:
            _call("cimrgp_cov_lml_grad", _dt(dt), cov, xd.data_ptr(), n, d, kp.ptr(), kp.ld, ad.data_ptr(), q, ell, SF2, NOISE,
                  out.data_ptr(), scratch.data_ptr(), _stream())
        assert _guards_are_nan(full, nout)
        outs.append(out.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "the scratch content or the run changed the bits"
    got = outs[0].cpu().numpy()
    assert np.isfinite(got).all()
    ratios = np.asarray(np.abs(np.asarray(got, dtype=cn.LD) - g) / cn.lml_grad_bound(g, w, s, UNIT[dt], n), dtype=np.float64)
    return np.array([ratios[0], ratios[1:-1].max(), ratios[-1]])          # sf | the length-scale entries | noise


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", DTS)
def test_gradient_contraction_entries_are_inside_their_own_bounds(ca, dt, cov, ard):
    """cimrgp_cov_lml_grad[_ard]: every output entry within ITS bound (not the largest entry's), finite, the same bits for
    NaN and for 1e300 in the scratch; K^-1 is NaN strictly above the diagonal (the kernel reads gc <= gr only); q up to
    the 8 padded columns of the alpha alpha^T loop."""
    worst = np.max([_run_grad(dt, cov, n, d, q, ard) for n, d, q in GRAD_SHAPES], axis=0)
    print("cov_lml_grad%s %s cov %d: worst err/bound sf %.2e, l %.2e, noise %.2e" % (("_ard" if ard else "", dt, cov) + tuple(worst)))
    assert worst.max() <= 1.0


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("cov", [0, 2])
@pytest.mark.parametrize("dt", DTS)
def test_gradient_contraction_past_1024_records(ca, dt, cov, ard):
    """n = 2945: 1128 tile records, so lml_grad_entry's loop `t, t + 1024, ..` makes its second trip.  Length-scales of 16:
    the setting at which tests/test_cov_host.py shows that dropping the records past 1024 exceeds every entry's bound."""
    n, d, q = GRAD_BIG
    assert len(cn.tile_ids(n)[0]) == 1128
    worst = _run_grad(dt, cov, n, d, q, ard, wide=True)
    print("cov_lml_grad%s %s cov %d n = %d: err/bound sf %.2e, l %.2e, noise %.2e" % (("_ard" if ard else "", dt, cov, n) + tuple(worst)))
    assert worst.max() <= 1.0


# --------------------------------------------------------------------------------------------------- small reductions ----
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("dt", DTS)
def test_logdet_half(ca, dt, n):
    """sum_i log L_ii (FP64 sums in both dtypes) against longdouble at (ceil(n / 1024) + 24) 2^-53 sum |log L_ii|; everything
    off the diagonal is NaN; an odd pitch gives the same bits."""
    diag = _f32(np.random.RandomState(n).uniform(0.5, 2.0, size=n))
    ref, sabs = cn.logdet_terms(diag)
    outs = []
    for ld in (_padded_ld(n), n if n % 2 else n + 1):
        lfull, lmat = _guarded(n * ld, TDT[dt])
        lmat[::ld + 1][:n] = _dev(diag, dt)
        full, out = _guarded(1, torch.float64)
        _call("cimrgp_logdet_half", _dt(dt), lmat.data_ptr(), n, ld, out.data_ptr(), _stream())
        assert _guards_are_nan(full, 1)
        outs.append(out.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    err, bnd = abs(cn.LD(float(outs[0][0])) - ref), cn.reduction_steps(n) * 2.0 ** -53 * float(sabs) + 1e-300
    print("logdet_half %s n = %d: err/bound %.3f" % (dt, n, float(err / bnd)))
    assert err <= bnd


@pytest.mark.parametrize("dt", DTS)
def test_add_diag_at_an_odd_pitch(ca, dt):
    n = 131
    k = _f32(np.random.RandomState(2).randn(n, n))
    noise = _dev([0.375], dt)
    res = []
    for layout in ODD_PITCH:
        kp = Placed(n, n, layout, dt, values=k)
        _call("cimrgp_add_diag", _dt(dt), kp.ptr(), n, kp.ld, noise.data_ptr(), _stream())
        assert kp.outside_is_nan()
        res.append((layout, [kp.mat()]))
    _same_bits_everywhere(res, "add_diag")
    want = k.astype(NPT[dt])
    want[np.diag_indices(n)] += NPT[dt](0.375)
    assert np.array_equal(_host(res[0][1][0]), want.astype(np.float64))


@pytest.mark.parametrize("n,q", [(1, 1), (1025, 3), (4097, 8)])
@pytest.mark.parametrize("dt", DTS)
def test_block_stats(ca, dt, n, q):
    """Column means and pooled variance of y = 1000 + noise of size 1 (a one-pass variance would lose every digit in FP32)
    against longdouble at (ceil(n q / 1024) + 24) u sum |terms|: |y_ic| / n for a mean, (y_ic - mean_c)^2 / (n q) for the
    variance."""
    y = _f32(1000.0 + np.random.RandomState(n + q).randn(n, q))
    ref, sabs = cn.block_stats_terms(y)
    yd = _dev(y, dt)
    outs = []
    for _ in range(2):
        full, out = _guarded(q + 1, TDT[dt])
        _call("cimrgp_block_stats", _dt(dt), yd.data_ptr(), None, n, q, out.data_ptr(), _stream())
        assert _guards_are_nan(full, q + 1)
        outs.append(out.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    got = _host(outs[0])
    assert np.isfinite(got).all()
    bnd = np.asarray(cn.reduction_steps(n * q) * UNIT[dt] * sabs, dtype=np.float64)
    err = np.asarray(np.abs(np.asarray(got, dtype=cn.LD) - ref), dtype=np.float64)
    print("block_stats %s (%d, %d): worst err/bound mean %.3f, variance %.3f"
          % (dt, n, q, float((err[:q] / bnd[:q]).max()), float(err[q] / bnd[q]) if bnd[q] > 0 else 0.0))
    assert np.all(err <= bnd)
