"""The memory footprint of the C ABI (include/cimrgp.h): which bytes each call reads and writes.

Every buffer a call touches lives inside a larger tensor, :class:`Guarded`: a guard of GUARD_BYTES before and after
it, a leading dimension wider than ``padded_ld(n)``, guard rows below the matrix, gaps between the blocks of a batched
arena.  Each element has a role:

  UNTOUCHED  neither read nor written: guards, padding columns, gaps, rows outside a layer's blocks, the strict upper
             triangle of an input factor / K^-1 (poisoned; must keep its bytes)
  JUNK       not read before it is written, may be written: scratch, workspaces, the strict upper triangle of K after a
             factorisation (poisoned; not checked afterwards)
  CONST      a const input: holds its value, must keep its bytes
  OUT        an output whose old contents are not read (poisoned)
  INOUT      an output that starts from a value (in-place input, accumulate = 1, info's 0x5A5A5A5A)

:func:`run_contract` runs a call three times -- poison 0 ("clean"), NaN and random finite values -- and asserts that
the outputs of the three runs are bitwise equal, that no UNTOUCHED or CONST element changed (compared through an
integer view, so NaN compares too), and leaves the buffers holding the outputs (equal to the clean run's).  The values
are then held to the FP64 oracle for n <= 6144 at the tolerances of the other GPU tests of the same entry point.

The entry points are called through ``cimrgp_amd._lib`` directly: the ``device.py`` wrappers allocate their own work
areas.  Importing this module does not touch the GPU (tests/test_buffer_contract_host.py imports the helper); only the
``dev`` fixture does.
"""

import numpy as np
import pytest
import scipy.linalg as sla

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_BYTES = 64 * 1024
UNTOUCHED, JUNK, CONST, OUT, INOUT = range(5)
ROLE_NAMES = ("untouched", "junk", "const", "out", "inout")
MODES = ("clean", "nan", "rand")
INFO_FILL = 0x5A5A5A5A
_INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int64: torch.int64, torch.int32: torch.int32,
        torch.uint8: torch.uint8}


def _ints(t):
    return t.view(_INT[t.dtype])


def wide_ld(cols):
    """A leading dimension (elements) wider than device.padded_ld(cols), a multiple of 16 elements."""
    return (int(cols) + 15) // 16 * 16 + 48


class Guarded(object):
    """``count`` elements of ``dtype`` between two guards of GUARD_BYTES; every element has a role (default
    UNTOUCHED).  ``ld`` (optional) is the row pitch of the 2-D views."""

    def __init__(self, name, count, dtype, device, ld=None):
        esz = torch.empty((), dtype=dtype).element_size()
        self.name, self.count, self.dtype, self.device, self.esz, self.ld = name, int(count), dtype, device, esz, ld
        self.g = GUARD_BYTES // esz
        total = 2 * self.g + self.count
        self.full = torch.zeros(total, dtype=dtype, device=device)
        self.role = torch.full((total,), UNTOUCHED, dtype=torch.uint8, device=device)
        self.init = None
        self.data = self.full[self.g:self.g + self.count]
        self.before = None

    def ptr(self, off=0):
        return self.data.data_ptr() + int(off) * self.esz

    def _2d(self, t, rows, ld, off):
        assert off + rows * ld <= self.count, (self.name, off, rows, ld, self.count)
        return t[self.g + off:self.g + off + rows * ld].view(rows, ld)

    def mat(self, rows, cols, ld=None, off=0):
        """(rows x cols) view of the payload at element ``off`` with pitch ``ld``."""
        ld = self.ld if ld is None else ld
        return self._2d(self.full, rows, ld, off)[:, :cols]

    def mark(self, role, rows, cols, ld=None, off=0, part="all", values=None):
        """Give the (rows x cols) region at ``off`` the role ``role``: all of it, its "lower" triangle (diagonal
        included), its strict "upper" triangle, or where a boolean (rows x cols) tensor is set.  ``values``: the
        region's contents for CONST / INOUT (the same in every run)."""
        ld = self.ld if ld is None else ld
        r = self._2d(self.role, rows, ld, off)[:, :cols]
        if isinstance(part, str):
            ii = torch.arange(rows, device=self.device)[:, None]
            jj = torch.arange(cols, device=self.device)[None, :]
            sel = {"all": None, "lower": jj <= ii, "upper": jj > ii}[part]
        else:
            sel = part.to(self.device)
        if sel is None:
            r.fill_(role)
        else:
            r.masked_fill_(sel, role)
        if values is not None:
            if self.init is None:
                self.init = torch.zeros_like(self.full)
            v = self._2d(self.init, rows, ld, off)[:, :cols]
            vals = torch.as_tensor(np.asarray(values) if not isinstance(values, torch.Tensor) else values)
            vals = vals.to(device=self.device, dtype=self.dtype).reshape(rows, cols)
            v.copy_(vals if sel is None else torch.where(sel, vals, v))
        return self

    def vec(self, role, n, off=0, values=None):
        return self.mark(role, 1, n, ld=n, off=off, values=values)

    def fill(self, mode, seed):
        """Poison every element for run ``mode``, then put the CONST / INOUT values in."""
        f = self.full
        if mode == "clean":
            f.zero_()
        elif mode == "nan":
            if f.dtype.is_floating_point:
                f.fill_(float("nan"))
            else:
                _ints(f).fill_(-1 if f.dtype != torch.uint8 else 255)
        else:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            if f.dtype.is_floating_point:
                f.copy_(torch.randn(f.numel(), generator=gen, device=self.device, dtype=f.dtype) * 100.0)
            else:
                hi = 256 if f.dtype == torch.uint8 else 2 ** 31 - 1
                f.copy_(torch.randint(0, hi, (f.numel(),), generator=gen, device=self.device, dtype=f.dtype))
        if self.init is not None:
            keep = (self.role == CONST) | (self.role == INOUT)
            f.copy_(torch.where(keep, self.init, f))
        self.before = f.clone()

    def _where(self, i):
        if i < self.g:
            return "the guard before it (element %d)" % (i - self.g)
        if i >= self.g + self.count:
            return "the guard after it (element +%d)" % (i - self.g - self.count)
        p = i - self.g
        rc = "" if not self.ld else " = row %d, column %d at ld %d" % (p // self.ld, p % self.ld, self.ld)
        return "payload element %d%s (%s)" % (p, rc, ROLE_NAMES[int(self.role[i])])

    def check_unchanged(self, mode):
        changed = _ints(self.full) != _ints(self.before)
        bad = changed & ((self.role == UNTOUCHED) | (self.role == CONST))
        if bool(bad.any()):
            idx = torch.nonzero(bad).flatten()
            raise AssertionError("%s: %d element(s) that must keep their bytes changed in the %s run, first at %s, last at %s"
                                 % (self.name, idx.numel(), mode, self._where(int(idx[0])), self._where(int(idx[-1]))))

    def outputs(self):
        return self.full[(self.role == OUT) | (self.role == INOUT)].clone()


def run_contract(bufs, call, sync=None):
    """Run ``call()`` clean, NaN-poisoned and randomly poisoned (module docstring); return nothing, leave the
    buffers holding the outputs."""
    sync = sync or (lambda: None)
    snaps = []
    for k, mode in enumerate(MODES):
        for i, b in enumerate(bufs):
            b.fill(mode, seed=7919 * k + 31 * i + 1)
        sync()
        call()
        sync()
        for b in bufs:
            b.check_unchanged(mode)
        snaps.append([b.outputs() for b in bufs])
    for i, b in enumerate(bufs):
        for k in (1, 2):
            a, c = _ints(snaps[0][i]), _ints(snaps[k][i])
            if not torch.equal(a, c):
                diff = torch.nonzero(a != c).flatten()
                raise AssertionError("%s: %d output element(s) of the %s run differ from the clean run (first: output #%d)"
                                     % (b.name, diff.numel(), MODES[k], int(diff[0])))


# ---- GPU side ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


def _lib():
    from cimrgp_amd import _lib as L
    return L


def _call(rc, what):
    _lib().check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


TDT = {"f64": torch.float64, "f32": torch.float32}
NU = {1: 0.5, 2: 1.5, 3: 2.5}
CUDA = "cuda"


def _dt(tdt):
    return _lib().F64 if tdt == torch.float64 else _lib().F32


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / (np.max(np.abs(b)) + 1e-300))


def _round(a, tdt):
    """Host values as the device holds them."""
    return np.asarray(a, dtype=np.float32 if tdt == torch.float32 else np.float64).astype(np.float64)


def _host(t):
    return t.double().cpu().numpy()


def _kcov(xa, xb, cov, ell, sf2):
    if cov == 0:
        return oracle.rbf_gram(xa, xb, ell, sf2)
    d2 = ((xa[:, None, :] - xb[None, :, :]) ** 2).sum(-1)
    nu = NU[cov]
    t = np.sqrt(2 * nu) * np.sqrt(d2) / ell
    poly = {0.5: 1.0, 1.5: 1 + t, 2.5: 1 + t + t * t / 3}[nu]
    return sf2 * poly * np.exp(-t)


def _const_vec(name, a, tdt):
    """A guarded CONST vector holding ``a`` (flattened)."""
    a = a.reshape(-1) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a).reshape(-1)
    size = int(a.numel() if isinstance(a, torch.Tensor) else a.size)
    return Guarded(name, size, tdt, CUDA).vec(CONST, size, values=a)


def _out_vec(name, count, tdt, pre=None):
    b = Guarded(name, count, tdt, CUDA)
    return b.vec(INOUT if pre is not None else OUT, count, values=pre)


def _info(batch=1):
    return Guarded("info", batch, torch.int32, CUDA).vec(INOUT, batch, values=np.full(batch, INFO_FILL, dtype=np.int64))


def _factor_buf(name, n, tdt, extra_rows=3):
    """K / L: lower triangle OUT, strict upper JUNK, padding columns and guard rows UNTOUCHED."""
    ld = wide_ld(n)
    b = Guarded(name, (n + extra_rows) * ld, tdt, CUDA, ld=ld)
    b.mark(OUT, n, n, part="lower").mark(JUNK, n, n, part="upper")
    return b


def _ws_buf(n, tdt, role=JUNK, values=None):
    nbytes = int(_lib().load().cimrgp_potrf_workspace_bytes(_dt(tdt), int(n)))
    esz = torch.empty((), dtype=tdt).element_size()
    b = Guarded("workspace", max(nbytes // esz, 1), tdt, CUDA)
    b.nbytes = nbytes
    if nbytes:
        b.vec(role, nbytes // esz, values=values)
    return b


# ---- Gram ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lower_only", [False, True])
@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_gram_footprint(dev, dt, n, d, lower_only):
    """rbf_gram / cov_gram (four covariances): the lower triangle (everything with lower_only = 0) is written and
    nothing right of column n or below row n; lower_only = 1 may write above the diagonal inside the n x n block."""
    tdt = TDT[dt]
    rng = np.random.default_rng(n * 10 + d)
    x = _round(rng.uniform(-1.7, 1.7, size=(n, d)), tdt)
    xb = _const_vec("x", x, tdt)
    kb = Guarded("K", (n + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n))
    kb.mark(OUT, n, n, part="lower").mark(JUNK if lower_only else OUT, n, n, part="upper")
    lib = _lib().load()
    tol = 1e-13 if dt == "f64" else 2e-6
    for cov in (0, 1, 2, 3):
        def call():
            if cov == 0:
                _call(lib.cimrgp_rbf_gram(_dt(tdt), xb.ptr(), n, d, 0.37, 1.9, 0.05, kb.ptr(), kb.ld, int(lower_only), _stream()),
                      "cimrgp_rbf_gram")
            else:
                _call(lib.cimrgp_cov_gram(_dt(tdt), cov, xb.ptr(), n, d, 0.37, 1.9, 0.05, kb.ptr(), kb.ld, int(lower_only),
                                          _stream()), "cimrgp_cov_gram")
        run_contract([xb, kb], call, _sync)
        ref = _kcov(x, x, cov, 0.37, 1.9) + 0.05 * np.eye(n)
        got = _host(kb.mat(n, n))
        if lower_only:
            got, ref = np.tril(got), np.tril(ref)
        assert np.max(np.abs(got - ref)) / 1.95 < tol, cov


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("na,nb,d", [(77, 201, 2), (1, 65, 3), (130, 1, 1), (257, 63, 8)])
def test_cross_gram_footprint(dev, dt, na, nb, d):
    """rbf_cross / cov_cross: ragged na x nb at ld > nb; nothing right of column nb or below row na is touched."""
    tdt = TDT[dt]
    rng = np.random.default_rng(na + nb)
    xa = _round(rng.uniform(-1.5, 1.5, size=(na, d)), tdt)
    xbh = _round(rng.uniform(-1.5, 1.5, size=(nb, d)), tdt)
    ga, gb = _const_vec("xa", xa, tdt), _const_vec("xb", xbh, tdt)
    kab = Guarded("Kab", (na + 3) * wide_ld(nb), tdt, CUDA, ld=wide_ld(nb)).mark(OUT, na, nb)
    lib = _lib().load()
    tol = 1e-13 if dt == "f64" else 2e-6
    for cov in (0, 1, 2, 3):
        def call():
            if cov == 0:
                _call(lib.cimrgp_rbf_cross(_dt(tdt), ga.ptr(), na, gb.ptr(), nb, d, 0.8, 0.7, kab.ptr(), kab.ld, _stream()),
                      "cimrgp_rbf_cross")
            else:
                _call(lib.cimrgp_cov_cross(_dt(tdt), cov, ga.ptr(), na, gb.ptr(), nb, d, 0.8, 0.7, kab.ptr(), kab.ld, _stream()),
                      "cimrgp_cov_cross")
        run_contract([ga, gb, kab], call, _sync)
        assert np.max(np.abs(_host(kab.mat(na, nb)) - _kcov(xa, xbh, cov, 0.8, 0.7))) / 0.7 < tol, cov


# ---- factorisation -------------------------------------------------------------------------------------------------
def _chol_problem(n, tdt, seed):
    rng = np.random.default_rng(seed)
    x = _round(np.sort(rng.uniform(-2.0, 2.0, size=(n, 1)), axis=0), tdt)
    ell = 0.3 if n < 4096 else 0.05
    noise = 0.01 if tdt == torch.float64 else 0.1
    return rng, x, ell, 1.0, noise


def _check_factor(l_gpu, x, ell, sf2, noise, tdt):
    n = x.shape[0]
    if tdt == torch.float64:
        lref, info = oracle.potrf_lower(oracle.rbf_gram(x, None, ell, sf2, noise))
        assert info == 0
        assert _rel(l_gpu, lref) < 1e-10
        return lref
    # FP32: backward error of the factor (tests/test_gpu_kernels.py), formed in FP64 on the device
    k = torch.from_numpy(oracle.rbf_gram(x, None, ell, sf2, noise)).cuda()
    l64 = torch.from_numpy(l_gpu).cuda()
    resid = float(torch.linalg.norm(l64 @ l64.t() - k) / torch.linalg.norm(k))
    assert resid < (2e-5 if n <= 1025 else 8 * n * float(np.finfo(np.float32).eps)), resid
    return None


@pytest.mark.parametrize("dt,n", [("f64", 1), ("f64", 65), ("f64", 257), ("f64", 1025), ("f64", 4864), ("f64", 5377),
                                  ("f64", 6144), ("f64", 9001), ("f64", 10240), ("f32", 257), ("f32", 5632), ("f32", 8192)])
def test_potrf_footprint(dev, dt, n):
    """potrf behind rbf_gram(lower_only = 1) into a K whose upper triangle is poisoned: one-queue sizes, the
    look-ahead schedule (above 4864), ragged last panels, the persistent update (multiples of 128, n >= 4096), the
    paired far updates (above 8192).  The workspace is exactly cimrgp_potrf_workspace_bytes."""
    tdt = TDT[dt]
    rng, x, ell, sf2, noise = _chol_problem(n, tdt, n)
    xb = _const_vec("x", x, tdt)
    kb = _factor_buf("K", n, tdt)
    ws = _ws_buf(n, tdt)
    info = _info()
    lib = _lib().load()

    def call():
        _call(lib.cimrgp_rbf_gram(_dt(tdt), xb.ptr(), n, 1, ell, sf2, noise, kb.ptr(), kb.ld, 1, _stream()), "cimrgp_rbf_gram")
        _call(lib.cimrgp_potrf(_dt(tdt), kb.ptr(), n, kb.ld, ws.ptr(), ws.nbytes, info.ptr(), _stream()), "cimrgp_potrf")
    run_contract([xb, kb, ws, info], call, _sync)
    assert int(info.data[0]) == 0
    if n <= 6144:
        _check_factor(np.tril(_host(kb.mat(n, n))), x, ell, sf2, noise, tdt)


@pytest.mark.parametrize("dt,n,m", [("f64", 700, 130), ("f64", 5632, 2050), ("f64", 6000, 33), ("f32", 5632, 130)])
def test_potrf_rows_footprint(dev, dt, n, m):
    """potrf_rows: the carried rows B (m x n at ldb > n) are updated in place, their padding and the rows below
    are not touched."""
    tdt = TDT[dt]
    rng, x, ell, sf2, noise = _chol_problem(n, tdt, n + m)
    bmat = _round(rng.normal(size=(m, n)), tdt)
    xb = _const_vec("x", x, tdt)
    kb = _factor_buf("K", n, tdt)
    ws = _ws_buf(n, tdt)
    info = _info()
    bb = Guarded("B", (m + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n)).mark(INOUT, m, n, values=bmat)
    lib = _lib().load()

    def call():
        _call(lib.cimrgp_rbf_gram(_dt(tdt), xb.ptr(), n, 1, ell, sf2, noise, kb.ptr(), kb.ld, 1, _stream()), "cimrgp_rbf_gram")
        _call(lib.cimrgp_potrf_rows(_dt(tdt), kb.ptr(), n, kb.ld, ws.ptr(), ws.nbytes, info.ptr(), bb.ptr(), m, bb.ld, _stream()),
              "cimrgp_potrf_rows")
    run_contract([xb, kb, ws, info, bb], call, _sync)
    assert int(info.data[0]) == 0
    lgpu = np.tril(_host(kb.mat(n, n)))
    _check_factor(lgpu, x, ell, sf2, noise, tdt)
    lref = lgpu if tdt == torch.float32 else oracle.potrf_lower(oracle.rbf_gram(x, None, ell, sf2, noise))[0]
    want = sla.solve_triangular(lref, bmat.T, lower=True).T
    got = _host(bb.mat(m, n))
    if tdt == torch.float64:
        assert _rel(got, want) < 1e-9
    else:
        assert float(np.linalg.norm(got - want) / np.linalg.norm(want)) < 2e-3


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,batch,m", [(130, 3, 2), (2049, 2, 0), (1300, 24, 2)])
def test_potrf_rows_batched_footprint(dev, dt, n, batch, m):
    """potrf_rows_batched with gaps between the matrices, the workspaces and the row blocks (strides larger than
    needed) and a guarded info array."""
    tdt = TDT[dt]
    esz = torch.empty((), dtype=tdt).element_size()
    ld = wide_ld(n)
    k_stride = (n + 2) * ld
    ws_bytes = int(_lib().load().cimrgp_potrf_workspace_bytes(_dt(tdt), n))
    ws_stride = (ws_bytes + 15) // 16 * 16 + 4096
    b_stride = (m + 2) * ld
    rng = np.random.default_rng(n + batch)
    xs = [_round(np.sort(rng.uniform(-2, 2, size=(n, 1)), axis=0), tdt) for _ in range(batch)]
    ells = [0.3 + 0.1 * i for i in range(batch)]
    kar = Guarded("K arena", batch * k_stride, tdt, CUDA, ld=ld)
    war = Guarded("workspace arena", batch * ws_stride // esz, tdt, CUDA)
    bar = Guarded("B arena", max(batch * b_stride, 1), tdt, CUDA, ld=ld)
    info = _info(batch)
    bmats = [_round(rng.normal(size=(m, n)), tdt) for _ in range(batch)]
    for i in range(batch):
        kar.mark(INOUT, n, n, off=i * k_stride, part="lower", values=np.tril(oracle.rbf_gram(xs[i], None, ells[i], 1.0, 0.05)))
        kar.mark(JUNK, n, n, off=i * k_stride, part="upper")
        war.vec(JUNK, ws_bytes // esz, off=i * ws_stride // esz)
        if m:
            bar.mark(INOUT, m, n, off=i * b_stride, values=bmats[i])
    lib = _lib().load()

    def call():
        _call(lib.cimrgp_potrf_rows_batched(_dt(tdt), kar.ptr(), n, ld, k_stride, war.ptr(), ws_stride, info.ptr(),
                                            bar.ptr() if m else None, m, ld if m else 0, b_stride if m else 0, batch, _stream()),
              "cimrgp_potrf_rows_batched")
    run_contract([kar, war, bar, info], call, _sync)
    assert info.data.cpu().tolist() == [0] * batch
    tol = 1e-10 if dt == "f64" else 5e-4
    for i in range(batch):
        lref, _ = oracle.potrf_lower(oracle.rbf_gram(xs[i], None, ells[i], 1.0, 0.05))
        assert _rel(np.tril(_host(kar.mat(n, n, off=i * k_stride))), lref) < tol, i
        if m:
            want = sla.solve_triangular(lref, bmats[i].T, lower=True).T
            assert _rel(_host(bar.mat(m, n, off=i * b_stride)), want) < 10 * tol, i


# ---- solves --------------------------------------------------------------------------------------------------------
def _factored(dev, n, tdt, seed):
    """A factor and its workspace, made with the wrappers; returned as host values to seed CONST buffers."""
    rng, x, ell, sf2, noise = _chol_problem(n, tdt, seed)
    xd = dev.to_device(x, tdt, CUDA)
    kbuf = dev.rbf_gram(xd, ell, sf2, noise, lower_only=True)
    ws, info = dev.potrf(kbuf, n)
    _sync()
    assert int(info.item()) == 0
    lower = torch.tril(kbuf[:n, :n]).clone()
    esz = torch.empty((), dtype=tdt).element_size()
    return rng, lower, ws.view(tdt)[:ws.numel() // esz].clone()


def _const_factor(lower, n, tdt, extra_rows=3):
    """A guarded input factor: lower triangle CONST, everything else (strict upper, padding, guard rows) UNTOUCHED."""
    ld = wide_ld(n)
    return Guarded("L", (n + extra_rows) * ld, tdt, CUDA, ld=ld).mark(CONST, n, n, part="lower", values=lower)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [65, 1025, 5377, 6144])
def test_solves_footprint(dev, dt, n):
    """potrs (z NULL and given), solve_lt and trsm_rows against a const factor whose strict upper triangle and
    padding are poisoned, a const workspace and scratch of exactly 2 q n elements; held to the FP64 triangular
    solves with the same factor."""
    tdt = TDT[dt]
    rng, lower, wsv = _factored(dev, n, tdt, n)
    lgpu = lower.double().cpu().numpy()
    lb = _const_factor(lower, n, tdt)
    nbytes = int(_lib().load().cimrgp_potrf_workspace_bytes(_dt(tdt), n))
    ws = Guarded("workspace", wsv.numel(), tdt, CUDA).vec(CONST, wsv.numel(), values=wsv)
    lib = _lib().load()
    tol = {"f64": 1e-9, "f32": 5e-3}[dt]
    for q in (1, 8):
        r = _round(rng.normal(size=(n, q)), tdt)
        zref = sla.solve_triangular(lgpu, r, lower=True)
        aref = sla.solve_triangular(lgpu, zref, lower=True, trans="T")
        scratch = Guarded("scratch", 2 * q * n, tdt, CUDA).vec(JUNK, 2 * q * n)
        for want_z in (False, True):
            rhs = Guarded("rhs", n * q, tdt, CUDA).vec(INOUT, n * q, values=r)
            z = Guarded("z", n * q, tdt, CUDA).vec(OUT, n * q)
            bufs = [lb, ws, rhs, scratch] + ([z] if want_z else [])
            run_contract(bufs, lambda: _call(lib.cimrgp_potrs(_dt(tdt), lb.ptr(), n, lb.ld, ws.ptr(), rhs.ptr(), q,
                                                              z.ptr() if want_z else None, scratch.ptr(), _stream()),
                                             "cimrgp_potrs"), _sync)
            assert _rel(_host(rhs.data).reshape(n, q), aref) < tol, (q, want_z)
            if want_z:
                assert _rel(_host(z.data).reshape(n, q), zref) < tol, q
        zb = Guarded("z", n * q, tdt, CUDA).vec(INOUT, n * q, values=zref)
        run_contract([lb, ws, zb, scratch], lambda: _call(lib.cimrgp_solve_lt(_dt(tdt), lb.ptr(), n, lb.ld, ws.ptr(), zb.ptr(), q,
                                                                              scratch.ptr(), _stream()), "cimrgp_solve_lt"), _sync)
        assert _rel(_host(zb.data).reshape(n, q), sla.solve_triangular(lgpu, _round(zref, tdt), lower=True, trans="T")) < tol, q
    trsm_tol = {"f64": 1e-9, "f32": 3e-3}[dt]
    for m in (1, 17, 2050):
        b = _round(rng.normal(size=(m, n)), tdt)
        bb = Guarded("B", (m + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n)).mark(INOUT, m, n, values=b)
        run_contract([lb, ws, bb], lambda: _call(lib.cimrgp_trsm_rows(_dt(tdt), lb.ptr(), n, lb.ld, ws.ptr(), bb.ptr(), m, bb.ld,
                                                                      _stream()), "cimrgp_trsm_rows"), _sync)
        assert _rel(_host(bb.mat(m, n)), sla.solve_triangular(lgpu, b.T, lower=True).T) < trsm_tol, m
    assert nbytes == ws.count * ws.esz


def test_solve_lt_batched_footprint(dev):
    """solve_lt_batched, batch 5, n = 1300, q = 3: factors and workspaces at strides with gaps (poisoned, unread),
    scratch of exactly batch x 2 q n elements."""
    tdt, n, q, batch = torch.float64, 1300, 3, 5
    ld = wide_ld(n)
    l_stride = (n + 2) * ld
    ws_bytes = dev.potrf_workspace_bytes(n, tdt)
    ws_stride = (ws_bytes + 15) // 16 * 16 + 2048
    rng = np.random.default_rng(11)
    lar = Guarded("L arena", batch * l_stride, tdt, CUDA, ld=ld)
    war = Guarded("workspace arena", batch * ws_stride // 8, tdt, CUDA)
    lowers, zs = [], []
    for i in range(batch):
        _, lower, wsv = _factored(dev, n, tdt, 100 + i)
        lowers.append(lower.cpu().numpy())
        lar.mark(CONST, n, n, off=i * l_stride, part="lower", values=lower)
        war.vec(CONST, wsv.numel(), off=i * ws_stride // 8, values=wsv)
        zs.append(rng.normal(size=(n, q)))
    zb = _out_vec("z", batch * n * q, tdt, pre=np.stack(zs))
    scratch = Guarded("scratch", batch * 2 * q * n, tdt, CUDA).vec(JUNK, batch * 2 * q * n)
    lib = _lib().load()
    run_contract([lar, war, zb, scratch],
                 lambda: _call(lib.cimrgp_solve_lt_batched(_dt(tdt), lar.ptr(), n, ld, l_stride, war.ptr(), ws_stride, zb.ptr(), q,
                                                           scratch.ptr(), batch, _stream()), "cimrgp_solve_lt_batched"), _sync)
    got = _host(zb.data).reshape(batch, n, q)
    for i in range(batch):
        assert _rel(got[i], sla.solve_triangular(lowers[i], zs[i], lower=True, trans="T")) < 1e-8, i


# ---- prediction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ns", [1, 37, 1000])
def test_predict_footprint(dev, dt, ns):
    """predict_mean / cov_predict_mean (bias NULL and given, accumulate both ways) and predict_from_w (bias, mean,
    var, extra_var_dev each NULL and given, accumulate both ways); the accumulated outputs start from random values."""
    tdt = TDT[dt]
    n, d, q = 257, 2, 2
    rng = np.random.default_rng(ns)
    x = _round(rng.uniform(-1.7, 1.7, size=(n, d)), tdt)
    xs = _round(rng.uniform(-1.7, 1.7, size=(ns, d)), tdt)
    alpha = _round(rng.normal(size=(n, q)), tdt)
    bias = _round(np.array([0.25, -1.5]), tdt)
    gx, gxs, ga, gbias = _const_vec("x", x, tdt), _const_vec("xs", xs, tdt), _const_vec("alpha", alpha, tdt), _const_vec("bias", bias, tdt)
    lib = _lib().load()
    tol = {"f64": 1e-9, "f32": 2e-3}[dt]
    ell, sf2 = 0.4, 1.3
    for cov in (0, 3):
        kxs = _kcov(xs, x, cov, ell, sf2)
        for with_bias in (False, True):
            for acc in (0, 1):
                pre = _round(rng.normal(size=(ns, q)), tdt) if acc else None
                mean = _out_vec("mean", ns * q, tdt, pre=pre)
                bufs = [gx, gxs, ga, mean] + ([gbias] if with_bias else [])

                def call():
                    bp = gbias.ptr() if with_bias else None
                    if cov == 0:
                        _call(lib.cimrgp_predict_mean(_dt(tdt), gx.ptr(), n, d, ga.ptr(), q, gxs.ptr(), ns, ell, sf2, bp, mean.ptr(),
                                                      acc, _stream()), "cimrgp_predict_mean")
                    else:
                        _call(lib.cimrgp_cov_predict_mean(_dt(tdt), cov, gx.ptr(), n, d, ga.ptr(), q, gxs.ptr(), ns, ell, sf2, bp,
                                                          mean.ptr(), acc, _stream()), "cimrgp_cov_predict_mean")
                run_contract(bufs, call, _sync)
                want = kxs @ alpha + (bias if with_bias else 0.0) + (pre if acc else 0.0)
                assert _rel(_host(mean.data).reshape(ns, q), want) < tol, (cov, with_bias, acc)
    # predict_from_w
    w = _round(0.05 * rng.normal(size=(ns, n)), tdt)
    z = _round(rng.normal(size=(n, q)), tdt)
    gw = Guarded("W", (ns + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n)).mark(CONST, ns, n, values=w)
    gz = _const_vec("z", z, tdt)
    gev = _const_vec("extra_var", np.array([0.125]), tdt)
    for with_mean, with_var in ((True, True), (True, False), (False, True)):
        for with_bias in (False, True):
            for with_ev in (False, True):
                for acc in (0, 1):
                    mpre = _round(rng.normal(size=(ns, q)), tdt) if acc else None
                    vpre = _round(rng.uniform(0, 1, size=ns), tdt) if acc else None
                    mean = _out_vec("mean", ns * q, tdt, pre=mpre)
                    var = _out_vec("var", ns, tdt, pre=vpre)
                    bufs = [gw, gz] + ([mean] if with_mean else []) + ([var] if with_var else []) + \
                        ([gbias] if with_bias else []) + ([gev] if with_ev else [])
                    run_contract(bufs, lambda: _call(lib.cimrgp_predict_from_w(
                        _dt(tdt), gw.ptr(), ns, n, gw.ld, gz.ptr(), q, sf2, 0.5, gev.ptr() if with_ev else None,
                        gbias.ptr() if with_bias else None, mean.ptr() if with_mean else None, var.ptr() if with_var else None,
                        acc, _stream()), "cimrgp_predict_from_w"), _sync)
                    case = (with_mean, with_var, with_bias, with_ev, acc)
                    if with_mean:
                        want = w @ z + (bias if with_bias else 0.0) + (mpre if acc else 0.0)
                        assert _rel(_host(mean.data).reshape(ns, q), want) < tol, case
                    if with_var:
                        want = sf2 + 0.5 + (0.125 if with_ev else 0.0) - np.sum(w * w, axis=1) + (vpre if acc else 0.0)
                        assert float(np.max(np.abs(_host(var.data) - want))) / sf2 < tol, case


# ---- residual chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 70001])
def test_residual_chain_footprint(dev, dt, n):
    """block_stats (fbar NULL and given), residual, train_mean (accumulate both ways), noise_from_stats for
    q = 1, 3, 8; add_diag (everything but the n diagonal elements keeps its bytes) and logdet_half (everything off
    the diagonal poisoned) for n <= 1025 (an n x n matrix at n = 70001 would be 39 GB).  The FP32 statistics are held
    to an accuracy bar against the FP64 reference of the same (rounded) inputs."""
    tdt = TDT[dt]
    lib = _lib().load()
    D = _dt(tdt)
    rng = np.random.default_rng(n)
    f64 = dt == "f64"
    for q in (1, 3, 8):
        y = _round(rng.normal(size=(n, q)) * np.linspace(1.0, 3.0, q) + np.linspace(0.5, -2.0, q), tdt)
        fbar = _round(0.1 * rng.normal(size=(n, q)), tdt)
        gy, gf = _const_vec("y", y, tdt), _const_vec("fbar", fbar, tdt)
        for with_f in (False, True):
            stats = _out_vec("stats", q + 1, tdt)
            run_contract([gy, stats] + ([gf] if with_f else []),
                         lambda: _call(lib.cimrgp_block_stats(D, gy.ptr(), gf.ptr() if with_f else None, n, q, stats.ptr(), _stream()),
                                       "cimrgp_block_stats"), _sync)
            r = y - (fbar if with_f else 0.0)
            mu = r.mean(axis=0)
            pooled = float(np.mean((r - mu) ** 2))
            got = _host(stats.data)
            scale = np.sqrt(pooled) + np.abs(mu)
            if f64:
                np.testing.assert_allclose(got, np.r_[mu, pooled], rtol=1e-12, atol=1e-14 * float(np.max(scale)))
            else:
                assert np.all(np.abs(got[:q] - mu) <= 1e-5 * scale), (q, got[:q], mu)
                assert abs(got[q] - pooled) <= 1e-5 * pooled, (q, got[q], pooled)
        gs = _const_vec("stats", np.r_[mu, pooled], tdt)
        stats_h = _round(np.r_[mu, pooled], tdt)
        noise = _out_vec("noise", 1, tdt)
        run_contract([gs, noise], lambda: _call(lib.cimrgp_noise_from_stats(D, gs.ptr(), q, 0.01, 1e-8, noise.ptr(), _stream()),
                                                "cimrgp_noise_from_stats"), _sync)
        nz = float(_host(noise.data)[0])
        assert abs(nz - max(0.01 * stats_h[q], 1e-8)) <= (1e-12 if f64 else 3e-7) * max(0.01 * stats_h[q], 1e-8)
        gb = _const_vec("bias", stats_h[:q], tdt)
        rr = _out_vec("r", n * q, tdt)
        run_contract([gy, gf, gb, rr], lambda: _call(lib.cimrgp_residual(D, gy.ptr(), gf.ptr(), gb.ptr(), n, q, rr.ptr(), _stream()),
                                                     "cimrgp_residual"), _sync)
        rh = _host(rr.data).reshape(n, q)
        np.testing.assert_allclose(rh, y - fbar - stats_h[:q], rtol=0, atol=(1e-14 if f64 else 1e-5) * (1 + np.max(np.abs(y))))
        alpha = _round(rng.normal(size=(n, q)), tdt)
        gr, ga = _const_vec("r", rh, tdt), _const_vec("alpha", alpha, tdt)
        gn = _const_vec("noise", np.array([nz]), tdt)
        for acc in (0, 1):
            pre = _round(rng.normal(size=(n, q)), tdt) if acc else None
            out = _out_vec("train_out", n * q, tdt, pre=pre)
            run_contract([gr, ga, gb, gn, out],
                         lambda: _call(lib.cimrgp_train_mean(D, gr.ptr(), ga.ptr(), gb.ptr(), gn.ptr(), n, q, out.ptr(), acc, _stream()),
                                       "cimrgp_train_mean"), _sync)
            want = rh - nz * alpha + stats_h[:q] + (pre if acc else 0.0)
            np.testing.assert_allclose(_host(out.data).reshape(n, q), want, rtol=1e-12 if f64 else 1e-5,
                                       atol=(1e-13 if f64 else 1e-5) * (1 + np.max(np.abs(want))))
    if n > 1025:
        return
    ld = wide_ld(n)
    kvals = _round(rng.normal(size=(n, n)), tdt)
    eye = torch.eye(n, dtype=torch.bool)
    kb = Guarded("K", (n + 3) * ld, tdt, CUDA, ld=ld).mark(CONST, n, n, values=kvals).mark(INOUT, n, n, part=eye, values=kvals)
    gn = _const_vec("noise", np.array([0.375]), tdt)
    run_contract([kb, gn], lambda: _call(lib.cimrgp_add_diag(D, kb.ptr(), n, ld, gn.ptr(), _stream()), "cimrgp_add_diag"), _sync)
    npdt = np.float64 if f64 else np.float32
    assert np.array_equal(np.diag(_host(kb.mat(n, n))), (np.diag(kvals).astype(npdt) + npdt(0.375)).astype(np.float64))
    diag = _round(rng.uniform(0.5, 2.0, size=n), tdt)
    lb = Guarded("L", (n + 3) * ld, tdt, CUDA, ld=ld).mark(CONST, n, n, part=eye, values=np.diag(diag))
    out = _out_vec("logdet", 1, torch.float64)
    run_contract([lb, out], lambda: _call(lib.cimrgp_logdet_half(D, lb.ptr(), n, ld, out.ptr(), _stream()), "cimrgp_logdet_half"),
                 _sync)
    want = float(np.sum(np.log(diag)))
    assert abs(float(out.data[0]) - want) <= (1e-10 if f64 else 1e-5) * max(1.0, abs(want))


# ---- syrk_lower ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n,k", [("f64", 1, 1), ("f64", 33, 5), ("f64", 127, 17), ("f64", 300, 250), ("f64", 1000, 100),
                                    ("f64", 4096, 256), ("f64", 4096, 512), ("f64", 6144, 768), ("f32", 300, 250),
                                    ("f32", 4096, 256)])
def test_syrk_lower_footprint(dev, dt, n, k):
    """syrk_lower on a nonzero C with [k, lda) of A poisoned: the lower triangle is C - A A^T; the strict upper
    triangle is not read, and is not written outside the 128 x 128 diagonal blocks (the persistent update -- f64,
    n a multiple of 128, k = 256 or 512, n >= 4096 -- stores diagonal tiles whole; include/cimrgp.h)."""
    tdt = TDT[dt]
    rng = np.random.default_rng(n + k)
    c = _round(rng.normal(size=(n, n)), tdt)
    a = _round(rng.normal(size=(n, k)), tdt)
    ldc, lda = wide_ld(n), wide_ld(k)
    ii = torch.arange(n)[:, None]
    jj = torch.arange(n)[None, :]
    diag_blocks = (jj > ii) & (jj // 128 == ii // 128)
    cb = Guarded("C", (n + 3) * ldc, tdt, CUDA, ld=ldc).mark(INOUT, n, n, part="lower", values=c).mark(JUNK, n, n, part=diag_blocks)
    ab = Guarded("A", (n + 3) * lda, tdt, CUDA, ld=lda).mark(CONST, n, k, values=a)
    lib = _lib().load()
    run_contract([cb, ab], lambda: _call(lib.cimrgp_syrk_lower(_dt(tdt), cb.ptr(), ldc, ab.ptr(), lda, n, k, _stream()),
                                         "cimrgp_syrk_lower"), _sync)
    want = np.tril(c - a @ a.T)
    assert _rel(np.tril(_host(cb.mat(n, n))), want) < (1e-12 if dt == "f64" else 1e-5)


# ---- LML gradient --------------------------------------------------------------------------------------------------
def _grad_ref(x, kinv, alpha, cov, ell, sf2, noise, ard):
    """1/2 tr((alpha alpha^T - q K^-1) dK/dtheta) w.r.t. log sf2, log ell (or each log l_k; x pre-scaled), log noise."""
    q = alpha.shape[1]
    g = alpha @ alpha.T - q * kinv
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    out = []
    if cov == 0:
        k = sf2 * np.exp(-0.5 * d2 / ell ** 2)
        out.append(0.5 * np.sum(g * k))
        if ard:
            out += [0.5 * np.sum(g * k * (x[:, c][:, None] - x[:, c][None, :]) ** 2) for c in range(x.shape[1])]
        else:
            out.append(0.5 * np.sum(g * k * d2 / ell ** 2))
    else:
        nu = NU[cov]
        r = np.sqrt(d2)
        t = np.sqrt(2 * nu) * r / ell
        v = np.exp(-t)
        k = sf2 * {0.5: 1.0, 1.5: 1 + t, 2.5: 1 + t + t * t / 3}[nu] * v
        out.append(0.5 * np.sum(g * k))
        if ard:
            with np.errstate(divide="ignore", invalid="ignore"):
                a = {0.5: np.where(r > 0, sf2 * v / np.where(r > 0, r, 1), 0.0), 1.5: 3 * sf2 * v, 2.5: 5 * sf2 * (1 + t) * v / 3}[nu]
            out += [0.5 * np.sum(g * a * (x[:, c][:, None] - x[:, c][None, :]) ** 2) for c in range(x.shape[1])]
        else:
            out.append(0.5 * np.sum(g * {0.5: sf2 * t * v, 1.5: sf2 * t * t * v, 2.5: sf2 * t * t * (1 + t) * v / 3}[nu]))
    out.append(0.5 * noise * np.trace(g))
    return np.array(out)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,d", [(65, 1), (300, 3)])
def test_lml_grad_footprint(dev, dt, n, d):
    """lml_grad, lml_grad_ard, cov_lml_grad, cov_lml_grad_ard: K^-1's strict upper triangle and padding poisoned and
    unread, scratch of exactly cimrgp_lml_grad_scratch_bytes, the 3 or d + 2 output doubles guarded."""
    tdt = TDT[dt]
    rng = np.random.default_rng(n + d)
    x = _round(rng.uniform(-1.5, 1.5, size=(n, d)), tdt)
    y = np.sin(2 * x[:, :1]) + 0.1 * rng.normal(size=(n, 2))
    ell, sf2, noise = 0.8, 1.1, 0.05
    lib = _lib().load()
    sbytes = int(lib.cimrgp_lml_grad_scratch_bytes(n))
    assert sbytes % 8 == 0
    scratch = Guarded("scratch", sbytes // 8, torch.float64, CUDA).vec(JUNK, sbytes // 8)
    tol = 1e-9 if dt == "f64" else 1e-3
    for cov in (0, 1, 2, 3):
        for ard in (False, True):
            xin = x / np.array([0.7, 1.3, 0.9][:d]) if ard else x
            xin = _round(xin, tdt)
            k = _kcov(xin, xin, cov, 1.0 if ard else ell, sf2) + noise * np.eye(n)
            kinv = np.linalg.inv(k)
            kinv = _round(0.5 * (kinv + kinv.T), tdt)
            alpha = _round(np.linalg.solve(k, y), tdt)
            kb = _const_factor(np.tril(kinv), n, tdt)
            gx, ga = _const_vec("x", xin, tdt), _const_vec("alpha", alpha, tdt)
            nout = d + 2 if ard else 3
            out = _out_vec("grad", nout, torch.float64)
            D = _dt(tdt)

            def call():
                if ard and cov == 0:
                    rc = lib.cimrgp_lml_grad_ard(D, gx.ptr(), n, d, kb.ptr(), kb.ld, ga.ptr(), 2, sf2, noise, out.ptr(), scratch.ptr(), _stream())
                elif ard:
                    rc = lib.cimrgp_cov_lml_grad_ard(D, cov, gx.ptr(), n, d, kb.ptr(), kb.ld, ga.ptr(), 2, sf2, noise, out.ptr(),
                                                     scratch.ptr(), _stream())
                elif cov == 0:
                    rc = lib.cimrgp_lml_grad(D, gx.ptr(), n, d, kb.ptr(), kb.ld, ga.ptr(), 2, ell, sf2, noise, out.ptr(), scratch.ptr(),
                                             _stream())
                else:
                    rc = lib.cimrgp_cov_lml_grad(D, cov, gx.ptr(), n, d, kb.ptr(), kb.ld, ga.ptr(), 2, ell, sf2, noise, out.ptr(),
                                                 scratch.ptr(), _stream())
                _call(rc, "lml gradient")
            run_contract([kb, gx, ga, out, scratch], call, _sync)
            want = _grad_ref(xin, kinv, alpha, cov, 1.0 if ard else ell, sf2, noise, ard)
            assert _rel(_host(out.data), want) < tol, (cov, ard)


# ---- layers --------------------------------------------------------------------------------------------------------
def _layer_rows(rng, batch, n, d, q, gap=5, lead=7):
    rows = lead + batch * (n + gap) + 3
    x = rng.uniform(-1.7, 1.7, size=(rows, d))
    y = np.stack([np.sin(3 * x[:, 0] + c) + 0.2 * x[:, -1] for c in range(q)], axis=1) + 0.05 * rng.normal(size=(rows, q)) + 0.5
    fbar = 0.1 * rng.normal(size=(rows, q))
    starts = [lead + b * (n + gap) for b in range(batch)]
    return rows, x, y, fbar, starts


def _rows_buf(name, rows, width, starts, n, tdt, role, values=None):
    """A layer array (rows x width, contiguous): the rows of the blocks get ``role``, the rest stays UNTOUCHED."""
    b = Guarded(name, rows * width, tdt, CUDA, ld=width)
    for s in starts:
        b.mark(role, n, width, off=s * width, values=None if values is None else values[s:s + n])
    return b


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("n", [130, 1300])
@pytest.mark.parametrize("cov", [0, 3])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_layer_footprint(dev, dt, cov, n, q, shared):
    """layer_fit[_cov], layer_predict[_cov] and layer_lml_grad_cov on a batch of 3 blocks at NON-adjacent starts:
    rows between and around the blocks (x, y, fbar, train_out, xs, mean, var) are poisoned and neither read nor
    written; arenas with gaps; shared_bias / shared_noise given and NULL."""
    tdt = TDT[dt]
    f64 = dt == "f64"
    esz = 8 if f64 else 4
    D = _dt(tdt)
    lib = _lib().load()
    batch, d, ns = 3, 2, 77
    rng = np.random.default_rng(n * 10 + q + 100 * cov)
    rows, x, y, fbar, starts = _layer_rows(rng, batch, n, d, q)
    x, y, fbar = _round(x, tdt), _round(y, tdt), _round(fbar, tdt)
    ell, sf2 = 0.4, 1.3
    noise_frac = 0.01 if f64 else 0.2
    sbias = _round(np.array([0.1, -0.2, 0.3][:q]), tdt)
    snoise = _round(np.array([0.05]), tdt)
    gx = _rows_buf("x", rows, d, starts, n, tdt, CONST, x)
    gy = _rows_buf("y", rows, q, starts, n, tdt, CONST, y)
    gf = _rows_buf("fbar", rows, q, starts, n, tdt, CONST, fbar)
    tpre = _round(rng.normal(size=(rows, q)), tdt)
    gt = _rows_buf("train_out", rows, q, starts, n, tdt, INOUT, tpre)
    gst = Guarded("starts", batch, torch.int64, CUDA).vec(CONST, batch, values=np.array(starts))
    gsb, gsn = _const_vec("shared_bias", sbias, tdt), _const_vec("shared_noise", snoise, tdt)
    ld = wide_ld(n)
    k_stride = (n + 2) * ld
    ws_bytes = int(lib.cimrgp_potrf_workspace_bytes(D, n))
    ws_stride = (ws_bytes + 15) // 16 * 16 + 1024
    kar = Guarded("K arena", batch * k_stride, tdt, CUDA, ld=ld)
    war = Guarded("workspace arena", batch * ws_stride // esz, tdt, CUDA)
    for b in range(batch):
        kar.mark(OUT, n, n, off=b * k_stride, part="lower").mark(JUNK, n, n, off=b * k_stride, part="upper")
        war.vec(JUNK, ws_bytes // esz, off=b * ws_stride // esz)
    info = _info(batch)
    ldr = wide_ld(n)
    rows_ar = Guarded("rows arena", batch * q * ldr, tdt, CUDA).vec(JUNK, batch * q * ldr)
    gz, galpha = _out_vec("z", batch * n * q, tdt), _out_vec("alpha", batch * n * q, tdt)
    gbias, gnoise = _out_vec("bias", batch * q, tdt), _out_vec("noise", batch, tdt)
    scratch = Guarded("scratch", batch * 2 * q * n, tdt, CUDA).vec(JUNK, batch * 2 * q * n)
    sb, sn = (gsb, gsn) if shared else (None, None)

    def fit():
        args = (gx.ptr(), gy.ptr(), gf.ptr(), gt.ptr(), gst.ptr(), batch, n, d, q, ell, sf2, -1.0, noise_frac, 1e-8 * sf2,
                sb.ptr() if shared else None, sn.ptr() if shared else None, kar.ptr(), ld, k_stride, war.ptr(), ws_stride,
                info.ptr(), rows_ar.ptr(), ldr, gz.ptr(), galpha.ptr(), gbias.ptr(), gnoise.ptr(), scratch.ptr(), _stream())
        if cov == 0:
            _call(lib.cimrgp_layer_fit(D, *args), "cimrgp_layer_fit")
        else:
            _call(lib.cimrgp_layer_fit_cov(D, cov, *args), "cimrgp_layer_fit_cov")
    run_contract([gx, gy, gf, gt, gst, kar, war, info, rows_ar, gz, galpha, gbias, gnoise, scratch] + ([gsb, gsn] if shared else []),
                 fit, _sync)
    assert info.data.cpu().tolist() == [0] * batch
    tol = {"L": 1e-10, "z": 1e-9, "alpha": 1e-8} if f64 else {"L": 5e-4, "z": 5e-3, "alpha": 5e-3}
    fits = []
    for b, s in enumerate(starts):
        r0 = y[s:s + n] - fbar[s:s + n]
        bias = sbias if shared else r0.mean(axis=0)
        r = r0 - bias
        noise = float(snoise[0]) if shared else max(noise_frac * float(np.mean(r * r)), 1e-8 * sf2)
        kf = _kcov(x[s:s + n], x[s:s + n], cov, ell, sf2)
        lref = sla.cholesky(kf + noise * np.eye(n), lower=True)
        zref = sla.solve_triangular(lref, r, lower=True)
        aref = sla.solve_triangular(lref, zref, lower=True, trans="T")
        fits.append((lref, bias, noise, r))
        assert _rel(np.tril(_host(kar.mat(n, n, off=b * k_stride))), lref) < tol["L"], b
        assert _rel(_host(gz.data).reshape(batch, n, q)[b], zref) < tol["z"], b
        assert _rel(_host(galpha.data).reshape(batch, n, q)[b], aref) < tol["alpha"], b
        assert np.max(np.abs(_host(gbias.data).reshape(batch, q)[b] - bias)) <= (1e-12 if f64 else 1e-5) * (1 + np.max(np.abs(bias)))
        assert abs(float(_host(gnoise.data)[b]) - noise) <= (1e-12 if f64 else 1e-5) * noise
        assert _rel(_host(gt.mat(n, q, off=s * q)), tpre[s:s + n] + kf @ aref + bias) < tol["alpha"], b

    # ---- prediction from the fit's outputs (now const inputs)
    lower = [torch.tril(kar.mat(n, n, off=b * k_stride)).clone() for b in range(batch)]
    wsv = [war.data[b * ws_stride // esz:b * ws_stride // esz + ws_bytes // esz].clone() for b in range(batch)]
    zv, bv, nv = gz.data.clone(), gbias.data.clone(), gnoise.data.clone()
    lar = Guarded("L arena", batch * k_stride, tdt, CUDA, ld=ld)
    wca = Guarded("workspace arena", batch * ws_stride // esz, tdt, CUDA)
    for b in range(batch):
        lar.mark(CONST, n, n, off=b * k_stride, part="lower", values=lower[b])
        wca.vec(CONST, ws_bytes // esz, off=b * ws_stride // esz, values=wsv[b])
    gzc, gbc, gnc = _const_vec("z", zv, tdt), _const_vec("bias", bv, tdt), _const_vec("noise", nv, tdt)
    trows = 4 + batch * (ns + 6) + 2
    t_starts = [4 + b * (ns + 6) for b in range(batch)]
    xs = _round(rng.uniform(-1.7, 1.7, size=(trows, d)), tdt)
    gxs = _rows_buf("xs", trows, d, t_starts, ns, tdt, CONST, xs)
    gts = Guarded("t_starts", batch, torch.int64, CUDA).vec(CONST, batch, values=np.array(t_starts))
    ldw = wide_ld(n)
    w_stride = (ns + 2) * ldw
    war_w = Guarded("W arena", batch * w_stride, tdt, CUDA, ld=ldw)
    for b in range(batch):
        war_w.mark(JUNK, ns, n, off=b * w_stride)
    mpre = _round(rng.normal(size=(trows, q)), tdt)
    vpre = _round(rng.uniform(0, 1, size=(trows, 1)), tdt)
    gm = _rows_buf("mean", trows, q, t_starts, ns, tdt, INOUT, mpre)
    gv = _rows_buf("var", trows, 1, t_starts, ns, tdt, INOUT, vpre)
    for with_noise in (False, True):
        def predict():
            args = (gx.ptr(), gst.ptr(), n, d, gxs.ptr(), gts.ptr(), ns, batch, ell, sf2, lar.ptr(), ld, k_stride, wca.ptr(), ws_stride,
                    gzc.ptr(), q, gbc.ptr(), gnc.ptr() if with_noise else None, war_w.ptr(), ldw, w_stride, gm.ptr(), gv.ptr(), _stream())
            if cov == 0:
                _call(lib.cimrgp_layer_predict(D, *args), "cimrgp_layer_predict")
            else:
                _call(lib.cimrgp_layer_predict_cov(D, cov, *args), "cimrgp_layer_predict_cov")
        run_contract([gx, gst, gxs, gts, lar, wca, gzc, gbc, war_w, gm, gv] + ([gnc] if with_noise else []), predict, _sync)
        ptol = 1e-8 if f64 else 5e-3
        for b, (s, t) in enumerate(zip(starts, t_starts)):
            lref, bias, noise, r = fits[b]
            ks = _kcov(xs[t:t + ns], x[s:s + n], cov, ell, sf2)
            wref = sla.solve_triangular(lref, ks.T, lower=True).T
            mwant = mpre[t:t + ns] + wref @ sla.solve_triangular(lref, r, lower=True) + bias
            vwant = vpre[t:t + ns, 0] + sf2 - np.sum(wref * wref, axis=1) + (noise if with_noise else 0.0)
            assert _rel(_host(gm.mat(ns, q, off=t * q)), mwant) < ptol, (b, with_noise)
            assert float(np.max(np.abs(_host(gv.mat(ns, 1, off=t))[:, 0] - vwant))) / sf2 < (1e-9 if f64 else 5e-3), (b, with_noise)

    # ---- the layer objective
    kinv_ar = Guarded("K^-1 arena", batch * k_stride, tdt, CUDA, ld=ld)
    for b in range(batch):
        kinv_ar.mark(OUT, n, n, off=b * k_stride, part="lower").mark(JUNK, n, n, off=b * k_stride, part="upper")
    sbytes = int(lib.cimrgp_layer_lml_grad_scratch_bytes(D, n, q, batch))
    lscratch = Guarded("scratch", sbytes, torch.uint8, CUDA).vec(JUNK, sbytes)
    lout = _out_vec("out", 4 * batch, torch.float64)
    info2 = _info(batch)
    lnoise = 0.05
    run_contract([gx, gy, gf, gst, kar, kinv_ar, war, info2, lscratch, lout] + ([gsb] if shared else []),
                 lambda: _call(lib.cimrgp_layer_lml_grad_cov(D, cov, gx.ptr(), gy.ptr(), gf.ptr(), gst.ptr(), batch, n, d, q, ell, sf2,
                                                             lnoise, gsb.ptr() if shared else None, kar.ptr(), ld, k_stride,
                                                             kinv_ar.ptr(), war.ptr(), ws_stride, info2.ptr(), lscratch.ptr(),
                                                             lout.ptr(), _stream()), "cimrgp_layer_lml_grad_cov"), _sync)
    assert info2.data.cpu().tolist() == [0] * batch
    got = _host(lout.data).reshape(batch, 4)
    for b, s in enumerate(starts):
        r0 = y[s:s + n] - fbar[s:s + n]
        r = r0 - (sbias if shared else r0.mean(axis=0))
        k = _kcov(x[s:s + n], x[s:s + n], cov, ell, sf2) + lnoise * np.eye(n)
        chol = sla.cholesky(k, lower=True)
        alpha = sla.cho_solve((chol, True), r)
        kinv = sla.cho_solve((chol, True), np.eye(n))
        lml = -0.5 * np.sum(r * alpha) - q * np.sum(np.log(np.diag(chol))) - 0.5 * n * q * np.log(2 * np.pi)
        grad = _grad_ref(x[s:s + n], kinv, alpha, cov, ell, sf2, lnoise, False)
        assert abs(got[b, 0] - lml) <= (1e-9 if f64 else 1e-3) * abs(lml), b
        assert _rel(got[b, 1:], grad) < (1e-7 if f64 else 1e-3), b


# ---- posterior calls -----------------------------------------------------------------------------------------------
def _posterior_problem(n, ns, q, d, tdt, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(n, d))
    x = _round(x[np.argsort(x[:, 0])], tdt)
    y = _round(np.stack([np.sin(2 * x[:, 0] + c) for c in range(q)], axis=1) + 0.1 * rng.normal(size=(n, q)), tdt)
    xs = _round(rng.uniform(-2.0, 2.0, size=(ns, d)), tdt)
    return rng, x, y, xs


class _PosteriorSet(object):
    """One guarded buffer set of cimrgp_block_posterior[_staged]."""

    def __init__(self, x, y, xs, tdt, acc, rng):
        n, d = x.shape
        q, ns = y.shape[1], xs.shape[0]
        self.n, self.d, self.q, self.ns, self.tdt = n, d, q, ns, tdt
        self.x, self.y, self.xs = _const_vec("x", x, tdt), _const_vec("y", y, tdt), _const_vec("xs", xs, tdt)
        self.k = _factor_buf("K", n, tdt)
        self.ws = _ws_buf(n, tdt)
        self.info = _info()
        self.w = Guarded("W", (ns + q + 3) * wide_ld(n), tdt, CUDA, ld=wide_ld(n)).mark(OUT, ns + q, n)
        self.alpha, self.z = _out_vec("alpha", n * q, tdt), _out_vec("z", n * q, tdt)
        self.scratch = Guarded("scratch", 2 * q * n, tdt, CUDA).vec(JUNK, 2 * q * n)
        self.mpre = _round(rng.normal(size=(ns, q)), tdt) if acc else None
        self.vpre = _round(rng.uniform(0, 1, size=ns), tdt) if acc else None
        self.mean, self.var = _out_vec("mean", ns * q, tdt, pre=self.mpre), _out_vec("var", ns, tdt, pre=self.vpre)
        self.acc = acc

    def bufs(self):
        return [self.x, self.y, self.xs, self.k, self.ws, self.info, self.w, self.alpha, self.z, self.scratch, self.mean, self.var]

    def args(self, ell, sf2, noise, add_noise):
        return (_dt(self.tdt), self.x.ptr(), self.n, self.d, self.y.ptr(), self.q, self.xs.ptr(), self.ns, ell, sf2, noise,
                self.k.ptr(), self.k.ld, self.ws.ptr(), self.ws.nbytes, self.info.ptr(), self.w.ptr(), self.w.ld, self.alpha.ptr(),
                self.z.ptr(), self.scratch.ptr(), self.mean.ptr(), self.var.ptr(), int(add_noise), self.acc)

    def results(self):
        n, q, ns = self.n, self.q, self.ns
        return [torch.tril(self.k.mat(n, n)).clone(), self.w.mat(ns + q, n).clone(), self.alpha.data.clone(), self.z.data.clone(),
                self.mean.data.clone(), self.var.data.clone()]

    def check_oracle(self, x, y, xs, ell, sf2, noise, add_noise):
        f64 = self.tdt == torch.float64
        fit = oracle.block_fit(x, y, ell, sf2, noise)
        om, ov = oracle.block_predict(x, fit, xs, ell, sf2, True)
        if add_noise:
            ov = ov + noise
        q, ns = self.q, self.ns
        mean = _host(self.mean.data).reshape(ns, q) - (self.mpre if self.acc else 0.0)
        var = _host(self.var.data) - (self.vpre if self.acc else 0.0)
        assert _rel(_host(self.alpha.data).reshape(-1, q), fit["alpha"]) < (1e-8 if f64 else 5e-3)
        assert _rel(mean, om) < (1e-8 if f64 else 2e-3)
        assert float(np.max(np.abs(var - ov))) / sf2 < (1e-9 if f64 else 2e-3)


@pytest.mark.parametrize("dt,n,ns,q,d,acc", [("f64", 300, 70, 2, 2, 0), ("f64", 5377, 70, 2, 1, 1), ("f32", 1100, 130, 3, 1, 1)])
def test_block_posterior_footprint(dev, dt, n, ns, q, d, acc):
    """block_posterior: K, W (ns + q rows), alpha, z, mean, var written inside their bounds; scratch exactly
    2 q n elements; the workspace exactly cimrgp_potrf_workspace_bytes."""
    tdt = TDT[dt]
    rng, x, y, xs = _posterior_problem(n, ns, q, d, tdt, n + ns)
    ell, sf2, noise = (0.3 if d == 2 else 0.05), 1.2, (0.02 if dt == "f64" else 0.1)
    s = _PosteriorSet(x, y, xs, tdt, acc, rng)
    lib = _lib().load()
    run_contract(s.bufs(), lambda: _call(lib.cimrgp_block_posterior(*s.args(ell, sf2, noise, acc), _stream()), "cimrgp_block_posterior"),
                 _sync)
    assert int(s.info.data[0]) == 0
    s.check_oracle(x, y, xs, ell, sf2, noise, acc)


@pytest.mark.parametrize("n", [5632, 8192])
def test_block_posterior_staged_footprint(dev, n):
    """block_posterior_staged on cimrgp_front_queue / the caller's stream / cimrgp_solve_queue over two buffer sets in
    rotation, two independent blocks enqueued back to back as bench.py does (n = 8192, ns = 130, q = 2 is its shape).
    While the first block's factorisation is in flight the second normally factors its early panels on the front queue;
    the test cannot force that path, it runs it as the benchmark does.  The first block is bitwise equal to the
    one-stream cimrgp_block_posterior of the same block (same stream, same layout).  The second is bitwise equal too
    unless it took the early panels, which group the trailing updates differently (include/cimrgp.h): then it agrees
    to rounding (1e-10 relative) and matches the oracle.  At n = 5632 the first block matches the oracle as well."""
    tdt, ns, q = torch.float64, 130, 2
    ell, sf2, noise = 0.1, 1.0, 0.01
    lib = _lib().load()
    probs = [_posterior_problem(n, ns, q, 1, tdt, n + b) for b in range(2)]
    sets = [_PosteriorSet(p[1], p[2], p[3], tdt, 0, p[0]) for p in probs]
    cur = torch.cuda.current_stream()
    fq, sq = dev.front_queue(cur), dev.solve_queue(cur)

    def call():
        for s in sets:
            _call(lib.cimrgp_block_posterior_staged(*s.args(ell, sf2, noise, 0), fq.cuda_stream, cur.cuda_stream, sq.cuda_stream),
                  "cimrgp_block_posterior_staged")
    run_contract(sets[0].bufs() + sets[1].bufs(), call, _sync)
    got = [s.results() for s in sets]
    assert [int(s.info.data[0]) for s in sets] == [0, 0]
    for b, s in enumerate(sets):
        run_contract(s.bufs(), lambda: _call(lib.cimrgp_block_posterior(*s.args(ell, sf2, noise, 0), cur.cuda_stream),
                                             "cimrgp_block_posterior"), _sync)
        ref = s.results()
        same = all(torch.equal(_ints(g), _ints(r)) for g, r in zip(got[b], ref))
        if b == 0:
            assert same
        elif not same:
            for name, g, r in zip(("L", "W", "alpha", "z", "mean", "var"), got[b], ref):
                assert float((g - r).abs().max() / r.abs().max()) < 1e-10, name
            for t, g in zip((s.k.mat(n, n), s.w.mat(ns + q, n), s.alpha.data, s.z.data, s.mean.data, s.var.data), got[b]):
                if t.dim() == 2 and t.shape[0] == n and t.shape[1] == n:
                    t.copy_(torch.where(torch.ones(n, n, dtype=torch.bool, device=CUDA).tril(), g, t))
                else:
                    t.copy_(g)
            s.check_oracle(probs[b][1], probs[b][2], probs[b][3], ell, sf2, noise, 0)
    if n <= 6144:
        sets[0].check_oracle(probs[0][1], probs[0][2], probs[0][3], ell, sf2, noise, 0)


# ---- reduced-rank path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,d,m,q", [(257, 2, 30, 2), (4099, 3, 17, 3)])
def test_reduced_rank_footprint(dev, dt, n, d, m, q):
    """laplace_basis, basis_moments (fbar / fvar NULL and given; scratch exactly
    cimrgp_basis_moments_scratch_bytes) and basis_apply (accumulate both ways)."""
    from oracle.reduced import laplace_basis
    tdt = TDT[dt]
    D = _dt(tdt)
    lib = _lib().load()
    rng = np.random.default_rng(n + m)
    x = _round(rng.uniform(-1.2, 1.2, size=(n, d)), tdt)
    interval = 1.05 * np.max(np.abs(x), axis=0) + 0.01
    phi, _ = laplace_basis(x, interval, m)
    gx = _const_vec("x", x, tdt)
    giv = _const_vec("interval", interval, torch.float64)
    gphi = _out_vec("phi", n * m, tdt)
    run_contract([gx, giv, gphi], lambda: _call(lib.cimrgp_laplace_basis(D, gx.ptr(), n, d, giv.ptr(), m, gphi.ptr(), _stream()),
                                                "cimrgp_laplace_basis"), _sync)
    assert np.max(np.abs(_host(gphi.data).reshape(n, m) - phi)) < (1e-12 if dt == "f64" else 2e-5) * max(1.0, m)
    y = _round(rng.normal(size=(n, q)) + 3.0, tdt)
    fbar = _round(rng.normal(size=(n, q)), tdt)
    fvar = _round(rng.uniform(0, 1, size=n), tdt)
    eau = rng.normal(size=(q, m)) * 0.1
    gy, gf, gfv, ge = _const_vec("y", y, tdt), _const_vec("fbar", fbar, tdt), _const_vec("fvar", fvar, tdt), _const_vec("eau", eau, torch.float64)
    sbytes = int(lib.cimrgp_basis_moments_scratch_bytes(n, m, q))
    assert sbytes % 8 == 0
    scratch = Guarded("scratch", sbytes // 8, torch.float64, CUDA).vec(JUNK, sbytes // 8)
    rec = m * q + 2 * m + q + 2
    for latent in (False, True):
        out = _out_vec("moments", rec, torch.float64)
        run_contract([gx, giv, gy, ge, out, scratch] + ([gf, gfv] if latent else []),
                     lambda: _call(lib.cimrgp_basis_moments(D, gx.ptr(), n, d, giv.ptr(), m, gy.ptr(), gf.ptr() if latent else None,
                                                            gfv.ptr() if latent else None, ge.ptr(), q, out.ptr(), scratch.ptr(), _stream()),
                                   "cimrgp_basis_moments"), _sync)
        got = out.data.cpu().numpy()
        r0 = y - (fbar if latent else 0.0) - phi @ eau.T
        tol, scale = 1e-9, float(np.sqrt(n)) * 10
        proj = phi.T @ r0
        assert np.max(np.abs(got[:m * q].reshape(m, q) - proj)) < tol * scale * (1 + np.max(np.abs(proj)))
        assert np.max(np.abs(got[m * q:m * q + m] - phi.sum(0))) < tol * scale
        assert _rel(got[m * q + m:m * q + 2 * m], (phi * phi).sum(0)) < tol
        assert np.max(np.abs(got[m * q + 2 * m:m * q + 2 * m + q] - r0.sum(0))) < tol * n
        assert abs(got[m * q + 2 * m + q] - np.sum(r0 * r0)) < tol * np.sum(r0 * r0)
        assert abs(got[-1] - (fvar.sum() if latent else 0.0)) < tol * n
    bias, c2 = rng.normal(size=q), rng.uniform(0, 1, size=m)
    gb, gc = _const_vec("bias", bias, torch.float64), _const_vec("c2", c2, torch.float64)
    tol = (1e-11 if dt == "f64" else 1e-5) * m
    for acc in (0, 1):
        mpre = _round(rng.normal(size=(n, q)), tdt) if acc else None
        vpre = _round(rng.uniform(0, 1, size=n), tdt) if acc else None
        mean, var = _out_vec("mean", n * q, tdt, pre=mpre), _out_vec("var", n, tdt, pre=vpre)
        run_contract([gx, giv, ge, gb, gc, mean, var],
                     lambda: _call(lib.cimrgp_basis_apply(D, gx.ptr(), n, d, giv.ptr(), m, ge.ptr(), q, gb.ptr(), gc.ptr(), 0.25,
                                                          mean.ptr(), var.ptr(), acc, _stream()), "cimrgp_basis_apply"), _sync)
        assert np.max(np.abs(_host(mean.data).reshape(n, q) - (bias + phi @ eau.T + (mpre if acc else 0.0)))) < 2 * tol
        assert np.max(np.abs(_host(var.data) - (0.25 + (phi * phi) @ c2 + (vpre if acc else 0.0)))) < 2 * tol
