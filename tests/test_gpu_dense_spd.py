"""The factorisation, the carried rows, the solves, the batched sweeps and the entries that build their own Gram matrix on
dense, well-conditioned SPD matrices: every 256-tile of L carries weight >= 1e-3 of max |L|, so a far-update tile that
is skipped, applied twice, reads the wrong operand block or loses a race fails here -- on the suite's other matrices
(RBF Gram of sorted points, ell = 0.05: numerically banded) it changes nothing a tolerance can see.

Matrices, acceptance rules and the case tables (which name the schedule path and the threshold each case straddles) are
in tests/dense_spd.py; tests/test_dense_spd_host.py shows that the rules pass the clean blocked algorithms and fail
every mutant of one tile's update by one panel.  In short: FP64 by the derived componentwise residual bound (rho <= 1,
the worst tile is reported), FP32 by forward error against the FP64 oracle of the same FP32-rounded inputs, at most
8 times the reference FP32 routine's.  K is formed on the device from the uploaded G (n x 32), rounded into the
library's buffer and READ BACK from it: the oracle and every residual use that matrix.  The oracle is LAPACK on the host
up to n = 6144 and torch.linalg on the device above; the oracle's solves and the FP32 reference solves are torch.linalg.

Both precisions pass.  FP32 did not at first: "what these tests found" below has the eight checks that missed the margin,
the cause and what was changed in the library.

With CIMRGP_DENSE_SPD_RECORD set to a file name every case appends one JSON line of its figures to it.
"""
import numpy as np
import pytest

import dense_spd as ds
import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TDT = {"f64": torch.float64, "f32": torch.float32}
NPDT = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def dev():
    from cimrgp_amd import device
    device.require_gpu()
    return device


@pytest.fixture(autouse=True)
def _release():
    """One matrix at a time: what a case allocated goes back to the device before the next one starts."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- plumbing ---------------------------------------------------------------------------------------------------------

def _lowrank_into(buf, n, seed, rec):
    """K = I + G G^T / r formed on the device in FP64 from the uploaded G, rounded into buf[:n, :n]; returns K as read back
    from the buffer's lower triangle (FP64, symmetric).  Asserts the cond bound from G's singular values."""
    g = ds.lowrank_spd(n, seed)
    kappa = ds.lowrank_cond_bound(n)
    cond = ds.lowrank_cond(g)
    rec["cond"], rec["cond_bound"] = cond, kappa
    assert cond <= kappa
    gd = torch.from_numpy(g).cuda()
    k = gd @ gd.t() / ds.RANK
    k.diagonal().add_(1.0)
    buf[:n, :n] = k.to(buf.dtype)
    del k
    return ds.sym_from_lower(buf[:n, :n].double())


def _oracle_factor(kin, n, dtype=np.float64):
    """The oracle's (FP64) or the reference's (FP32) factor of K, on the device: LAPACK on the host up to
    HOST_ORACLE_MAX, torch.linalg on the device above."""
    if n <= ds.HOST_ORACLE_MAX:
        return torch.from_numpy(ds.factor(kin.cpu().numpy().astype(dtype), dtype)).cuda()
    return torch.tril(ds.factor(kin, dtype))


def _rows_into(dev, m, n, tdt, seed_n=None):
    """B (m x n) standard normal in a padded buffer, and B as read back from it (FP64)."""
    bbuf = dev.alloc_matrix(m, n, tdt, "cuda")
    bbuf[:m, :n] = torch.from_numpy(ds.carried_rows(n if seed_n is None else seed_n, m)).to("cuda", tdt)
    return bbuf, bbuf[:m, :n].double().clone()


class Checks(object):
    """The figures of one case (one JSON line) and the rules it missed, by the name of the check.  A case is computed
    once (see _case): the tests that share it each hold it to some of its checks."""

    def __init__(self, **case):
        self.rec = dict(case)
        self.failed = []                                  # (name of the check, message)

    def tile_weight(self, lo):
        tw = ds.tile_weight(lo)
        self.rec["tile_weight"] = min(tw, self.rec.get("tile_weight", tw))
        if not tw >= ds.MIN_TILE_WEIGHT:
            self.failed.append(("tile_weight", "tile weight %.3e < %.0e: the matrix does not meet the condition"
                                % (tw, ds.MIN_TILE_WEIGHT)))

    def rho(self, what, rho, tile):
        self.rec[what] = dict(rho=rho, worst_tile=list(tile))
        if not rho <= 1.0:
            self.failed.append((what, ds.report(what, rho, tile)))

    def fp32(self, what, got, want, ref):
        dev_err, ref_err = ds.forward_error(got, want), ds.forward_error(ref, want)
        ratio = ds.fp32_ratio(dev_err, ref_err)
        self.rec[what] = dict(device_error=dev_err, reference_error=ref_err, ratio=ratio)
        if not ratio <= ds.FP32_MARGIN:
            self.failed.append((what, "%s: device error %.3e = %.2f x the reference's %.3e (limit %g)"
                                % (what, dev_err, ratio, ref_err, ds.FP32_MARGIN)))

    def cap(self, what, err, cap):
        self.rec[what] = dict(error=err, cap=cap)
        if not err < cap:
            self.failed.append((what, "%s: error %.3e, cap %.1e" % (what, err, cap)))

    def factor(self, what, dt, ldev, kin, lo, lref32, kappa):
        """The factor rule of ``dt``: ldev the library's lower triangle, lo the oracle's factor, lref32 the reference's.
        FP32 also records the same rule on the strictly lower entries alone (``what`` + "_strictly_lower"): the entries a
        wrong update tile moves, without the diagonal's own rounding."""
        if dt == "f64":
            self.rho(what, *ds.factor_rho(ldev, kin, kappa))
        else:
            self.fp32(what, ldev, lo, lref32)
            self.fp32(what + "_strictly_lower", torch.tril(ldev, -1), torch.tril(lo, -1), torch.tril(lref32, -1))

    def system(self, what, dt, got, lfac, b_in, kappa, lt=False):
        """The solve rule of ``dt`` for got L^T = b_in (``lt``: got L = b_in) with the library's own factor ``lfac`` (in
        its dtype) and the right-hand side as the library read it (FP64)."""
        if dt == "f64":
            self.rho(what, *ds.rows_rho(got, lfac, b_in, kappa, lt))
        else:
            want = ds.solve_rows(lfac.double(), b_in, np.float64, lt)
            ref = ds.solve_rows(lfac, b_in.float(), np.float32, lt)
            self.fp32(what, got, want, ref)

    def close(self):
        """The case is computed: its one line is recorded."""
        self.rec["missed"] = [name for name, _ in self.failed]
        ds.record(**self.rec)
        print(self.rec)
        return self

    def hold(self, judged=lambda name: True):
        """Assert the checks ``judged`` picks."""
        mine = [msg for name, msg in self.failed if judged(name)]
        assert not mine, "\n".join(mine)

    def done(self):
        self.close().hold()


_CASES = {}       # key -> the closed Checks of a case (figures only, no tensors): a case runs once however many tests hold it


def _case(key, compute):
    if key not in _CASES:
        _CASES[key] = compute().close()
    return _CASES[key]


def _kappa(n):
    return ds.lowrank_cond_bound(n)


def _check_inverse_blocks(ws, n, ref):
    """The inverted 64 x 64 diagonal blocks and the 256 x 256 blocks (L_pp^-1)^T left in the workspace, as
    test_potrf_f64_matches_lapack checks them."""
    nslab, npan = (n + 63) // 64, (n + 255) // 256
    flat = ws.view(torch.float64).cpu().numpy()
    inv = flat[:nslab * 4096].reshape(-1, 64, 64)
    for s in range(nslab):
        w = min(64, n - 64 * s)
        blk = ref[64 * s:64 * s + w, 64 * s:64 * s + w]
        np.testing.assert_allclose(inv[s][:w, :w] @ blk, np.eye(w), atol=1e-9)
        assert np.all(np.triu(inv[s], 1) == 0)
    inv_t = flat[nslab * 4096:nslab * 4096 + npan * 65536].reshape(npan, 256, 256)
    for p in range(npan):
        w = min(256, n - 256 * p)
        blk = ref[256 * p:256 * p + w, 256 * p:256 * p + w]
        np.testing.assert_allclose(inv_t[p][:w, :w].T @ blk, np.eye(w), atol=1e-8)
        assert np.all(np.tril(inv_t[p], -1) == 0)


# ---- what these tests found ----------------------------------------------------------------------------------------------
# FP64 passed everywhere with rho <= 1e-2: no wrong tile on any path.  FP32 at first missed the margin of 8 in eight checks
# (measured on an MI355X; HISTORY.md has the per-tile table):
#
#   cimrgp_potrf, n = 8192 / 9216 / 10240       factor 11.1 / 12.4 / 12.5 x the reference's (4.0 - 5.0 x from 5120 to 6144)
#   cimrgp_potrf_rows, n = 10240                the same factor, 12.5 x
#   cimrgp_trsm_rows, m = 15                    9.1 / 11.1 / 10.2 x at n = 700 / 2500 / 5632; m = 129 at n = 2500: 8.2 x
#
# The update kernels started their matrix-core accumulators as the C tile and subtracted the n products term by term, so an
# entry of size one took n roundings at ITS OWN ulp where LAPACK (a block's product accumulated from zero, one subtraction
# per block) takes n / nb.  In L only the diagonal is of size one: at n = 8192 its error grew with the column to 8.5e-6
# max |L| while every strictly lower entry stayed at 3.6e-7; in W = B L^-T every entry is of size one.  The FP32 64-tile
# update (gemm_tile.hpp, W <= 2: riders and small launches) and k_rows_step now accumulate the product apart from C / B:
# the factor is at 1.1 / 1.4 x at n = 5120 / 6144 and 3.6 / 4.7 / 5.6 x at 8192 / 9216 / 10240, trsm_rows at 2.3 x at most
# (profiles/dense_spd_errors.jsonl).  What is left above n = 6144 comes from the persistent kernel, which still chains on C
# (its C stream reloads the set it has just stored; HISTORY.md).  The FP32 factor is held to the rule on the whole factor and,
# as a check of this file's own beside it, on the strictly lower entries alone: the entries a wrong update tile moves, without
# the diagonal's own rounding.


def _params(cases, ident):
    """Every case in FP64 and FP32."""
    return [pytest.param(*(tuple(case) + (dt,)), id="%s-%s" % (ident(case), dt)) for case in cases for dt in ("f64", "f32")]


def _not_the_whole_factor(name):
    return name != "factor"


# ---- cimrgp_potrf ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,path,dt", _params(ds.POTRF, lambda c: "n%d" % c[0]))
def test_potrf_on_a_dense_matrix(dev, n, path, dt):
    """Every schedule path of cimrgp_potrf (dense_spd.POTRF names them) on a matrix whose every tile counts.  FP32: the
    factor rule on the whole factor and on its strictly lower entries."""
    c = Checks(entry="cimrgp_potrf", path=path, n=n, m=0, dtype=dt)
    tdt = TDT[dt]
    kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
    kin = _lowrank_into(kbuf, n, n, c.rec)
    ws, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    ldev = torch.tril(kbuf[:n, :n])
    del kbuf
    lo = _oracle_factor(kin, n)
    c.tile_weight(lo)
    lref32 = _oracle_factor(kin, n, np.float32) if dt == "f32" else None
    c.factor("factor", dt, ldev, kin, lo, lref32, _kappa(n))
    if n == 700 and dt == "f64":
        _check_inverse_blocks(ws, n, lo.cpu().numpy())
    c.done()


# ---- cimrgp_potrf_rows ---------------------------------------------------------------------------------------------------

def _potrf_rows_case(dev, n, m, path, dt):
    c = Checks(entry="cimrgp_potrf_rows", path=path, n=n, m=m, dtype=dt)
    tdt = TDT[dt]
    kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
    kin = _lowrank_into(kbuf, n, n, c.rec)
    bbuf, b_in = _rows_into(dev, m, n, tdt)
    ws, info = dev.potrf_rows(kbuf, n, bbuf, m)
    assert int(info.item()) == 0
    ldev = torch.tril(kbuf[:n, :n])
    del kbuf
    lo = _oracle_factor(kin, n)
    c.tile_weight(lo)
    lref32 = _oracle_factor(kin, n, np.float32) if dt == "f32" else None
    c.factor("factor", dt, ldev, kin, lo, lref32, _kappa(n))
    w = bbuf[:m, :n]
    if dt == "f64":
        c.rho("rows", *ds.rows_rho(w, ldev, b_in, _kappa(n)))
    else:
        # the whole operation against its reference: K and B in, W out
        c.fp32("rows", w, ds.solve_rows(lo, b_in), ds.solve_rows(lref32, b_in.float(), np.float32))
    return c


@pytest.mark.parametrize("n,m,path,dt", _params(ds.POTRF_ROWS, lambda c: "n%d-m%d" % c[:2]))
def test_potrf_rows_on_a_dense_matrix(dev, n, m, path, dt):
    """The carried rows W = B L^-T: their far update is W[:, far] -= W[:, panel] L[far, panel]^T, and here L[far, panel]
    is not zero.  (FP32: with the factor's strictly lower entries; the whole factor is test_potrf_rows_factor's.)"""
    _case(("potrf_rows", n, m, dt), lambda: _potrf_rows_case(dev, n, m, path, dt)).hold(_not_the_whole_factor)


@pytest.mark.parametrize("n,m,path,dt", _params(ds.POTRF_ROWS, lambda c: "n%d-m%d" % c[:2]))
def test_potrf_rows_factor(dev, n, m, path, dt):
    """The factor of the same run (not run again), by the rule on the whole factor."""
    _case(("potrf_rows", n, m, dt), lambda: _potrf_rows_case(dev, n, m, path, dt)).hold(lambda name: name == "factor")


# ---- solves on a dense factor -----------------------------------------------------------------------------------------------

def _solves_case(dev, n, dt):
    c = Checks(entry="solves", path="solves on a dense factor; " + ("bwd_pairs" if n > 5120 else "one-queue sizes"), n=n, m=0, dtype=dt)
    tdt, kappa = TDT[dt], _kappa(n)
    rng = np.random.default_rng(7 * n)
    kbuf = dev.alloc_matrix(n, n, tdt, "cuda")
    kin = _lowrank_into(kbuf, n, n, c.rec)
    ws, info = dev.potrf(kbuf, n)
    assert int(info.item()) == 0
    lfac = torch.tril(kbuf[:n, :n])
    lo = _oracle_factor(kin, n)
    c.tile_weight(lo)
    lref32 = _oracle_factor(kin, n, np.float32) if dt == "f32" else None
    c.factor("factor", dt, lfac, kin, lo, lref32, kappa)

    def normal(*shape):
        return torch.from_numpy(rng.standard_normal(shape)).to("cuda", tdt).contiguous()

    for q in ds.SOLVE_Q:
        rhs = normal(n, q)
        r_in = rhs.double().clone()
        z = dev.potrs(kbuf, n, ws, rhs, want_z=True)
        c.system("potrs_q%d_z" % q, dt, z.t(), lfac, r_in.t(), kappa)                        # L z = r
        c.system("potrs_q%d_alpha" % q, dt, rhs.t(), lfac, z.double().t(), kappa, lt=True)   # L^T alpha = z
    z0 = normal(n, 3)
    alpha = dev.solve_lt(kbuf, n, ws, z0.clone())
    c.system("solve_lt", dt, alpha.t(), lfac, z0.double().t(), kappa, lt=True)
    for m in ds.SOLVE_M:
        for lt, call in ((False, dev.trsm_rows), (True, dev.trsm_rows_lt)):
            bbuf = dev.alloc_matrix(m, n, tdt, "cuda")
            bbuf[:m, :n] = normal(m, n)
            b_in = bbuf[:m, :n].double().clone()
            call(kbuf, n, ws, bbuf, m)
            c.system("%s_m%d" % ("trsm_rows_lt" if lt else "trsm_rows", m), dt, bbuf[:m, :n], lfac, b_in, kappa, lt)
    # rows [r0, r0 + m) of L^-T: a ragged strip in the middle and the last strip
    r_mid, r_last = 256 * ((n // 256) // 2), (n - 1) // 256 * 256
    for name, r0, m in (("trtri_rows_middle", r_mid, min(129, n - r_mid)), ("trtri_rows_last", r_last, n - r_last)):
        out = dev.alloc_matrix(m, n, tdt, "cuda")
        out.fill_(float("nan"))
        dev.trtri_rows(kbuf, n, ws, r0, m, out=out)
        assert torch.isnan(out[:m, :r0]).all() and torch.isnan(out[:m, n:]).all()      # neither read nor written
        strip = torch.zeros((m, n), dtype=tdt, device="cuda")
        strip[:, r0:] = out[:m, r0:n]
        unit = torch.zeros((m, n), dtype=torch.float64, device="cuda")
        unit[torch.arange(m), r0 + torch.arange(m)] = 1.0
        c.system(name, dt, strip, lfac, unit, kappa)                                      # S L^T = rows of I
    # diag(K^-1): bit-equal across strip heights, and the oracle's
    d = [dev.kinv_diag(kbuf, n, ws, dev.kinv_diag_scratch_bytes(n, strip, tdt)) for strip in (256, 1024)]
    assert torch.equal(d[0].view(torch.uint8), d[1].view(torch.uint8))
    want = ds.kinv_diag(lo)
    if dt == "f64":
        c.cap("kinv_diag", ds.forward_error(d[0], want), ds.kinv_diag_bound(n, kappa))
    else:
        c.fp32("kinv_diag", d[0], want, ds.kinv_diag(lref32, np.float32))
    return c


def _is_trsm_rows(name):
    return name.startswith("trsm_rows_m")


@pytest.mark.parametrize("n,dt", _params([(n,) for n in ds.SOLVES_N], lambda c: "n%d" % c[0]))
def test_solves_on_a_dense_factor(dev, n, dt):
    """potrs (with want_z), solve_lt, trsm_rows_lt, trtri_rows and kinv_diag from a factor that has just passed the factor
    rule.  n = 5632 > 5120: the backward solves use the paired off-diagonal inverse blocks, which on a banded factor are
    zero.  Every solve is judged against the library's OWN factor (FP64: residual; FP32: the FP64 solve with that factor,
    and torch's FP32 solve with it as the reference), so the factor's error stays out of it; only diag(K^-1) is compared
    with the oracle's, which it is documented to equal (FP64: within dense_spd.kinv_diag_bound, which a one-tile mutant
    exceeds a thousandfold -- test_dense_spd_host.py)."""
    _case(("solves", n, dt), lambda: _solves_case(dev, n, dt)).hold(lambda name: not _is_trsm_rows(name))


@pytest.mark.parametrize("m", ds.SOLVE_M, ids=lambda m: "m%d" % m)
@pytest.mark.parametrize("n,dt", _params([(n,) for n in ds.SOLVES_N], lambda c: "n%d" % c[0]))
def test_trsm_rows_on_a_dense_factor(dev, n, dt, m):
    """cimrgp_trsm_rows with m rows, from the same run (not run again), each (n, m) on its own."""
    _case(("solves", n, dt), lambda: _solves_case(dev, n, dt)).hold(lambda name: name == "trsm_rows_m%d" % m)


# ---- batched -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ds.BATCHED_M)
@pytest.mark.parametrize("n,batch,path,dt", _params(ds.BATCHED, lambda c: "%dx%d" % (c[1], c[0])))
def test_batched_on_dense_matrices(dev, n, batch, path, dt, m):
    """cimrgp_potrf_rows_batched on its three paths, every block its own matrix, then solve_lt_batched,
    trsm_rows_lt_batched and kinv_diag_batched: each block by the single-matrix rules (the worst block's figures are
    recorded)."""
    c = Checks(entry="cimrgp_potrf_rows_batched", path=path, n=n, m=m, batch=batch, dtype=dt)
    tdt, kappa = TDT[dt], _kappa(n)
    rng = np.random.default_rng(100 * n + batch + m)
    ld = dev.padded_ld(n)
    karena = torch.empty((batch, n, ld), dtype=tdt, device="cuda")
    ws_bytes = (dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16
    ws_arena = torch.empty((batch, max(ws_bytes, 16)), dtype=torch.uint8, device="cuda")
    info = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    kins = [_lowrank_into(karena[i], n, ds.batch_seed(n, i), c.rec) for i in range(batch)]
    rows = b_in = None
    if m:
        rows = torch.zeros((batch, m, ld), dtype=tdt, device="cuda")
        rows[:, :, :n] = torch.from_numpy(rng.standard_normal((batch, m, n))).to("cuda", tdt)
        b_in = rows[:, :, :n].double().clone()
    dev.potrf_rows_batched(karena, n, ld, ws_arena, info, rows, m, ld if m else 0)
    assert info.cpu().tolist() == [0] * batch

    def normal(*shape):
        return torch.from_numpy(rng.standard_normal(shape)).to("cuda", tdt).contiguous()

    q, mm = 2, 5
    z = normal(batch, n, q)
    z_in = z.double().clone()
    dev.solve_lt_batched(karena, n, ld, ws_arena, z)
    barena = torch.zeros((batch, mm, ld), dtype=tdt, device="cuda")
    barena[:, :, :n] = normal(batch, mm, n)
    x_in = barena[:, :, :n].double().clone()
    dev.trsm_rows_lt_batched(karena, n, ws_arena, barena, mm)
    d = [dev.kinv_diag_batched(karena, n, ws_arena, batch * dev.kinv_diag_scratch_bytes(n, strip, tdt)) for strip in (256, n)]
    assert torch.equal(d[0].view(torch.uint8), d[1].view(torch.uint8))

    worst = {}
    for i in range(batch):
        ci = Checks()
        lfac = torch.tril(karena[i, :, :n])
        lo = _oracle_factor(kins[i], n)
        ci.tile_weight(lo)
        lref32 = _oracle_factor(kins[i], n, np.float32) if dt == "f32" else None
        ci.factor("factor", dt, lfac, kins[i], lo, lref32, kappa)
        if m:
            if dt == "f64":
                ci.rho("rows", *ds.rows_rho(rows[i, :, :n], lfac, b_in[i], kappa))
            else:
                ci.fp32("rows", rows[i, :, :n], ds.solve_rows(lo, b_in[i]), ds.solve_rows(lref32, b_in[i].float(), np.float32))
        ci.system("solve_lt_batched", dt, z[i].t(), lfac, z_in[i].t(), kappa, lt=True)
        ci.system("trsm_rows_lt_batched", dt, barena[i, :, :n], lfac, x_in[i], kappa, lt=True)
        want = ds.kinv_diag(lo)
        if dt == "f64":
            ci.cap("kinv_diag_batched", ds.forward_error(d[0][i], want), ds.kinv_diag_bound(n, kappa))
        else:
            ci.fp32("kinv_diag_batched", d[0][i], want, ds.kinv_diag(lref32, np.float32))
        c.failed += [(name, "block %d: %s" % (i, msg)) for name, msg in ci.failed]
        c.rec["tile_weight"] = min(ci.rec["tile_weight"], c.rec.get("tile_weight", 1.0))
        for key, val in ci.rec.items():
            if isinstance(val, dict):
                size = val.get("rho", val.get("ratio", val.get("error")))
                if key not in worst or size > worst[key][0]:
                    worst[key] = (size, dict(val, block=i))
    c.rec.update({key: val for key, (_, val) in worst.items()})
    c.done()


# ---- entries that build their own Gram matrix: the kernel form ----------------------------------------------------------------

ELL, SF2, NOISE = ds.KERNEL_ELL, ds.KERNEL_SF2, ds.KERNEL_NOISE


def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / (np.max(np.abs(b)) + 1e-300))


def _kernel_block(n, ns, q, seed):
    rng = np.random.default_rng(seed + 1)
    x = ds.kernel_dense_points(n, seed)
    y = np.stack([np.sin(2 * x[:, 0] + c) for c in range(q)], axis=1) + 0.1 * rng.normal(size=(n, q))
    xs = rng.uniform(-2.0, 2.0, size=(ns, 1))
    return x, y, xs


_KERNEL_ORACLE = {}      # (n, ns, q, seed) -> (alpha, mean, var, tile weight): computed once, shared, never changed


def _kernel_oracle(n, ns, q, seed):
    """oracle.block_fit / block_predict up to HOST_ORACLE_MAX; above it the same steps with torch.linalg in FP64 on the
    device (explicit differences for the squared distances, as oracle.rbf_gram)."""
    key = (n, ns, q, seed)
    if key not in _KERNEL_ORACLE:
        x, y, xs = _kernel_block(n, ns, q, seed)
        if n <= ds.HOST_ORACLE_MAX:
            fit = oracle.block_fit(x, y, ELL, SF2, NOISE)
            mean, var = oracle.block_predict(x, fit, xs, ELL, SF2, True)
            out = (fit["alpha"], mean, var, ds.tile_weight(fit["L"]))
        else:
            xd, yd, xsd = (torch.from_numpy(a).cuda() for a in (x, y, xs))
            k = SF2 * torch.exp((xd - xd.t()) ** 2 * (-0.5 / (ELL * ELL)))
            k.diagonal().add_(NOISE)
            low = ds.factor(k)
            del k
            z = torch.linalg.solve_triangular(low, yd, upper=False)
            alpha = torch.linalg.solve_triangular(low.t(), z, upper=True)
            ks = SF2 * torch.exp((xsd - xd.t()) ** 2 * (-0.5 / (ELL * ELL)))
            v = torch.linalg.solve_triangular(low, ks.t(), upper=False)
            out = (alpha.cpu().numpy(), (ks @ alpha).cpu().numpy(), (SF2 - (v * v).sum(0)).cpu().numpy(), ds.tile_weight(low))
        _KERNEL_ORACLE[key] = out
    return _KERNEL_ORACLE[key]


def _posterior_buffers(dev, n, ns, q, tdt):
    return dict(kbuf=dev.alloc_matrix(n, n, tdt, "cuda"), wbuf=dev.alloc_matrix(ns + q, n, tdt, "cuda"),
                ws=dev.potrf_workspace(n, tdt, "cuda"),
                alpha=torch.zeros((n, q), dtype=tdt, device="cuda"), z=torch.zeros((n, q), dtype=tdt, device="cuda"),
                scratch=torch.empty(2 * q * n, dtype=tdt, device="cuda"))


def _check_posterior(c, tag, alpha, mean, var, want):
    """The caps of test_block_posterior_one_call_matches_the_separate_calls_and_the_oracle."""
    oalpha, omean, ovar, tw = want
    c.rec["tile_weight"] = min(tw, c.rec.get("tile_weight", tw))
    if not tw >= ds.MIN_TILE_WEIGHT:
        c.failed.append("tile weight %.3e: the matrix does not meet the condition" % tw)
    c.cap(tag + "alpha", _relerr(alpha.cpu().numpy(), oalpha), 1e-8)
    c.cap(tag + "mean", _relerr(mean.cpu().numpy(), omean), 1e-8)
    c.cap(tag + "var", float(np.max(np.abs(var.cpu().numpy() - ovar))) / SF2, 1e-9)


@pytest.mark.parametrize("n,path", ds.BLOCK_POSTERIOR, ids=["n%d" % c[0] for c in ds.BLOCK_POSTERIOR])
def test_block_posterior_on_the_kernel_form(dev, n, path):
    tdt, ns, q = torch.float64, 130, 2
    c = Checks(entry="cimrgp_block_posterior", path=path, n=n, m=ns + q, dtype="f64")
    xd, yd, xsd = (dev.to_device(a, tdt, "cuda") for a in _kernel_block(n, ns, q, n))
    b = _posterior_buffers(dev, n, ns, q, tdt)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    mean = torch.zeros((ns, q), dtype=tdt, device="cuda")
    var = torch.zeros(ns, dtype=tdt, device="cuda")
    dev.block_posterior(xd, yd, xsd, ELL, SF2, NOISE, b["kbuf"], b["wbuf"], b["ws"], info, b["alpha"], b["z"], mean, var,
                        scratch=b["scratch"])
    assert int(info.item()) == 0
    _check_posterior(c, "", b["alpha"], mean, var, _kernel_oracle(n, ns, q, n))
    c.done()


@pytest.mark.parametrize("front", [False, True], ids=["plain", "front-queue"])
@pytest.mark.parametrize("n,path", ds.STAGED, ids=["n%d" % c[0] for c in ds.STAGED])
def test_block_posterior_staged_on_the_kernel_form(dev, n, path, front):
    """Three independent blocks over TWO rotating buffer sets, the solve stage on the context's idle queue and, with
    ``front``, the front end (and with it the early panels of the next block) on the context's chain queue: each block
    against the oracle."""
    tdt, ns, q = torch.float64, 130, 2
    nblocks, nsets = 3, 2
    c = Checks(entry="cimrgp_block_posterior_staged", path=path + ("; front queue (early panels)" if front else ""), n=n,
               m=ns + q, dtype="f64")
    blocks = [tuple(dev.to_device(a, tdt, "cuda") for a in _kernel_block(n, ns, q, n + b)) for b in range(nblocks)]
    sets = [_posterior_buffers(dev, n, ns, q, tdt) for _ in range(nsets)]
    infos = [torch.full((1,), 12345, dtype=torch.int32, device="cuda") for _ in range(nblocks)]
    means = [torch.zeros((ns, q), dtype=tdt, device="cuda") for _ in range(nblocks)]
    vars_ = [torch.zeros(ns, dtype=tdt, device="cuda") for _ in range(nblocks)]
    alphas = [None] * nblocks
    cur = torch.cuda.current_stream()
    sq = dev.solve_queue(cur)
    fq = dev.front_queue(cur) if front else cur
    torch.cuda.synchronize()
    for i, (xd, yd, xsd) in enumerate(blocks):
        b = sets[i % nsets]
        dev.block_posterior(xd, yd, xsd, ELL, SF2, NOISE, b["kbuf"], b["wbuf"], b["ws"], infos[i], b["alpha"], b["z"],
                            means[i], vars_[i], scratch=b["scratch"], streams=(fq, cur, sq))
        with torch.cuda.stream(sq):                  # behind this call's solve stage, ahead of the set's next use
            alphas[i] = b["alpha"].clone()
    torch.cuda.synchronize()
    assert [int(i.item()) for i in infos] == [0] * nblocks
    for i in range(nblocks):
        _check_posterior(c, "block%d_" % i, alphas[i], means[i], vars_[i], _kernel_oracle(n, ns, q, n + i))
    c.done()


def test_layer_fit_and_predict_on_the_kernel_form(dev):
    """cimrgp_layer_fit + cimrgp_layer_predict on one layer of 4 x 1300: every block's points cover [-2, 2] (the blocks
    are row ranges of the layer's arrays; nothing asks for the layer to be sorted), at the caps of
    test_layer_fit_and_predict_match_oracle."""
    nb, n, path = ds.LAYER
    d, q, ns = 1, 2, 77
    tdt = torch.float64
    c = Checks(entry="cimrgp_layer_fit+cimrgp_layer_predict", path=path, n=n, m=q, batch=nb, dtype="f64")
    rng = np.random.default_rng(nb * 1000 + n)
    starts = np.array([11 + i * n for i in range(nb)], dtype=np.int64)
    total = nb * n + 37
    x = rng.uniform(-2.0, 2.0, size=(total, d))
    for i, a in enumerate(starts):
        x[a:a + n] = ds.kernel_dense_points(n, ds.batch_seed(n, i))
    y = np.stack([np.sin(3 * x[:, 0] + k) for k in range(q)], axis=1) + 0.05 * rng.normal(size=(total, q))
    fbar = 0.1 * rng.normal(size=(total, q))
    xd, yd, fd = (dev.to_device(a, tdt, "cuda") for a in (x, y, fbar))
    train_out = torch.zeros_like(yd)
    ld = dev.padded_ld(n)
    karena = torch.empty((nb, n, ld), dtype=tdt, device="cuda")
    ws_bytes = max((dev.potrf_workspace_bytes(n, tdt) + 15) // 16 * 16, 16)
    ws_arena = torch.empty((nb, ws_bytes), dtype=torch.uint8, device="cuda")
    info = torch.zeros(nb, dtype=torch.int32, device="cuda")
    bias = torch.empty((nb, q), dtype=tdt, device="cuda")
    noise = torch.empty(nb, dtype=tdt, device="cuda")
    z = torch.empty((nb, n, q), dtype=tdt, device="cuda")
    alpha = torch.empty((nb, n, q), dtype=tdt, device="cuda")
    sd = torch.as_tensor(starts).cuda()
    dev.layer_fit(xd, yd, fd, train_out, sd, n, ELL, SF2, NOISE, 0.01, 1e-8 * SF2, None, None, karena, ws_arena, info,
                  bias, noise, z, alpha)
    torch.cuda.synchronize()
    assert int(info.abs().max().item()) == 0
    xs = rng.uniform(-2.0, 2.0, size=(nb * ns + 9, d))
    t_starts = np.array([3 + i * ns for i in range(nb)], dtype=np.int64)
    mean = torch.zeros((xs.shape[0], q), dtype=tdt, device="cuda")
    var = torch.zeros(xs.shape[0], dtype=tdt, device="cuda")
    dev.layer_predict(xd, sd, n, dev.to_device(xs, tdt, "cuda"), torch.as_tensor(t_starts).cuda(), ns, ELL, SF2, karena, ws_arena,
                      z, bias, noise, mean, var)
    torch.cuda.synchronize()
    tout, mh, vh = train_out.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    for i, (a, t) in enumerate(zip(starts, t_starts)):
        r0 = y[a:a + n] - fbar[a:a + n]
        ob = r0.mean(axis=0)
        fit = oracle.block_fit(x[a:a + n], r0 - ob, ELL, SF2, NOISE)
        c.tile_weight(fit["L"])
        tag = "block%d_" % i
        c.cap(tag + "bias", _relerr(bias[i].cpu().numpy(), ob), 1e-12)
        c.cap(tag + "noise", abs(float(noise[i].item()) - NOISE) / NOISE, 1e-12)
        c.cap(tag + "factor", _relerr(np.tril(karena[i, :, :n].cpu().numpy()), fit["L"]), 1e-10)
        c.cap(tag + "z", _relerr(z[i].cpu().numpy(), fit["z"]), 1e-9)
        c.cap(tag + "alpha", _relerr(alpha[i].cpu().numpy(), fit["alpha"]), 1e-8)
        c.cap(tag + "train", _relerr(tout[a:a + n], oracle.rbf_gram(x[a:a + n], None, ELL, SF2) @ fit["alpha"] + ob), 1e-8)
        om, ov = oracle.block_predict(x[a:a + n], fit, xs[t:t + ns], ELL, SF2, True)
        c.cap(tag + "mean", _relerr(mh[t:t + ns], om + ob), 1e-8)
        c.cap(tag + "var", float(np.max(np.abs(vh[t:t + ns] - (ov + NOISE)))) / SF2, 1e-9)
    c.done()
