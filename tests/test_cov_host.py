"""The tests of the dense covariance tests (tests/cov_numpy.py), on the host: a NumPy restatement of the device kernels in
their dtype and operation order (gram_lanes / Cov<COV>::value, k_predict_mean, k_lml_grad_tiles + k_lml_grad_final) stays
inside every bound over the input grid of the GPU file, and every mutant of that restatement exceeds one -- among them
one far entry off by a relative 1e-4, which the normwise caps of the older tests accept.

The worst ratios are printed (outside pytest's capture) and copied into tests/cov_numpy.py."""
import functools
import math

import numpy as np
import pytest

import cov_numpy as cn

FT = {"f32": np.float32, "f64": np.float64}
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
DIMS = (1, 2, 3, 8)
ELLS = (0.6, 2.0 ** -4, 16.0)
OFFSETS = (0.0, 1024.0)
SF2 = 1.375
NOISE = 0.05
#: the normwise caps of test_rbf_gram / test_cov_gram_and_cross_match_closed_form: max |err| / sf2
OLD_CAP = {"f32": 2e-6, "f64": 1e-13}
#: power-of-two length-scales: x / ell is exact
ARD_ELLS = np.array([0.5, 2.0, 1.0, 0.25, 4.0, 1.0, 0.5, 2.0])


def _say(capsys, text):
    with capsys.disabled():
        print("\n  " + text, end="")


# ------------------------------------------------------------------------------------- the kernels' arithmetic in NumPy ----
def cov_scale(cov, ell):
    """common.hpp: cov_scale, in host double."""
    return {0: -0.5 / (ell * ell), 1: 1.0 / ell, 2: math.sqrt(3.0) / ell, 3: math.sqrt(5.0) / ell}[cov]


def _poly(cov, t, ft):
    if cov == 1:
        return ft(1)
    if cov == 2:
        return ft(1) + t
    return ft(1) + t + t * t * ft(1.0 / 3.0)


def _sq_dist(xa, xb, ft, mutant=None):
    """(d2, first difference) of gram_lanes: the differences' squares added in dimension order in the dtype."""
    xa, xb = xa.astype(ft), xb.astype(ft)
    df0 = xa[:, None, 0] - xb[None, :, 0]
    if mutant == "expanded":
        sa, sb, dot = np.zeros(len(xa), ft), np.zeros(len(xb), ft), np.zeros((len(xa), len(xb)), ft)
        for e in range(xa.shape[1]):
            sa, sb = sa + xa[:, e] * xa[:, e], sb + xb[:, e] * xb[:, e]
            dot = dot + xa[:, None, e] * xb[None, :, e]
        return np.maximum(sa[:, None] + sb[None, :] - ft(2) * dot, ft(0)), df0
    d2 = np.zeros((len(xa), len(xb)), ft)
    for e in range(xa.shape[1]):
        df = xa[:, None, e] - xb[None, :, e]
        d2 = d2 + df * df
    return d2, df0


def dev_value(xa, xb, cov, ell, sf2, ft, mutant=None):
    """Cov<COV>::value on gram_lanes' d2."""
    d2, df0 = _sq_dist(xa, xb, ft, mutant)
    c, sf2 = ft(cov_scale(cov, ell)), ft(sf2)
    if cov == 0:
        return sf2 * np.exp(d2 * c)
    r = np.abs(df0) if xa.shape[1] == 1 else np.sqrt(d2)
    if mutant == "eps":
        r = np.sqrt(d2 + ft(1e-12))
    t = c * r
    return sf2 * _poly(cov, t, ft) * np.exp(-t)


def dev_mean(x, alpha, xs, cov, ell, sf2, ft, bias=None, prefill=None):
    """k_predict_mean: lane ph adds the products of j = ph, ph + 32, .. in order, then the bias and the 32 partial sums."""
    kv = dev_value(xs, x, cov, ell, sf2, ft)
    alpha = alpha.astype(ft)
    n, q = alpha.shape
    part = np.zeros((len(xs), cn.PM_PH, q), ft)
    for j0 in range(0, n, cn.PM_PH):
        j = np.arange(j0, min(n, j0 + cn.PM_PH))
        part[:, :len(j)] = part[:, :len(j)] + kv[:, j, None] * alpha[None, j, :]
    s = np.zeros((len(xs), q), ft) if bias is None else np.broadcast_to(bias.astype(ft), (len(xs), q)).copy()
    for p in range(cn.PM_PH):
        s = s + part[:, p]
    return s if prefill is None else prefill.astype(ft) + s


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): offsets 32, 16, .. 1; every lane ends with the sum."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v


def _records(terms):
    """(T, 64 rows, 64 columns) FP64 terms -> the T tile records: thread (ty, tx) adds rows ty, ty + 4, .. in order, wave_sum
    over tx, sum4 over ty."""
    t4 = terms.reshape(terms.shape[0], 16, 4, 64)
    s = np.zeros(t4[:, 0].shape)
    for i in range(16):
        s = s + t4[:, i]
    w = _butterfly(s)[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _final(records):
    """lml_grad_entry: thread t adds records t, t + 1024, ..; block_sum (wave_sum, then the 16 waves in order)."""
    pad = np.zeros(-(-len(records) // 1024) * 1024)
    pad[:len(records)] = records
    s = np.zeros(1024)
    for row in pad.reshape(-1, 1024):
        s = s + row
    waves = _butterfly(s.reshape(16, 64))[:, 0]
    out = 0.0
    for w in waves:
        out = out + w
    return out


def dev_lml_grad(x, kinv, alpha, q, cov, ell, sf2, noise, ard, ft, mutant=None, tile=0):
    """k_lml_grad_tiles + k_lml_grad_final.  ``ard``: x is already divided by the length-scales and ``ell`` is not read.
    ``kinv`` is read on and below the diagonal (the mutant "upper" reads the diagonal tile ``tile`` above it too).
    Mutants act on record ``tile``: "skip", "twice", "weight1", "upper"; "drop1024" loses the records past the first 1024 and
    "alpha5" column 5 of alpha."""
    n, d = x.shape
    ri, ci, wgt = cn.tile_layout(n)
    diag = wgt == 1
    wgt = wgt.astype(np.float64)
    if mutant == "skip":
        wgt[tile] = 0
    elif mutant == "twice":
        wgt[tile] *= 2
    elif mutant == "weight1":
        wgt[tile] = np.minimum(wgt[tile], 1)
    elif mutant == "upper":
        gr, gc = ri[tile, 0, 0] + np.arange(64)[:, None], ci[tile, 0, 0] + np.arange(64)[None, :]
        wgt[tile] = np.where((gr < n) & (gc < n) & (gc > gr), 2, wgt[tile])
    xf, af = x.astype(ft), alpha.astype(ft)
    xa, xb = xf[ri[:, :, 0]], xf[ci[:, 0, :]]
    dk2, d2 = [], np.zeros(wgt.shape, ft)
    for e in range(d):
        df = xa[:, :, None, e] - xb[:, None, :, e]
        dk2.append(df * df)
        d2 = d2 + dk2[-1]
    aa, ab = af[ri[:, :, 0]], af[ci[:, 0, :]]
    aat = np.zeros(wgt.shape, ft)
    for c in range(q):
        if not (mutant == "alpha5" and c == 5):
            aat = aat + aa[:, :, None, c] * ab[:, None, :, c]
    kin = np.where(wgt > 0, kinv.astype(ft)[ri, ci], ft(0))
    g = aat - ft(q) * kin
    c_, sf = ft(cov_scale(cov, 1.0 if ard else ell)), ft(sf2)
    if cov == 0:
        kf = sf * np.exp(d2 * c_)
        gk = g * kf
        gl = g * kf * d2 * ft(1.0 if ard else 1.0 / (ell * ell))
    else:
        r = np.abs(xa[:, :, None, 0] - xb[:, None, :, 0]) if d == 1 else np.sqrt(d2)
        t = c_ * r
        v = np.exp(-t)
        kf = sf * _poly(cov, t, ft) * v
        third = ft(1.0 / 3.0)
        if cov == 1:
            with np.errstate(divide="ignore", invalid="ignore"):
                fa = np.where(r > 0, sf * c_ * v / np.where(r > 0, r, ft(1)), ft(0))
            fl = sf * t * v
        elif cov == 2:
            fa, fl = c_ * c_ * sf * v, sf * t * t * v
        else:
            fa, fl = c_ * c_ * sf * (ft(1) + t) * v * third, sf * t * t * (ft(1) + t) * v * third
        gk, gl = g * fa, g * fl
    cols = [(g * kf).astype(np.float64) * wgt]
    if ard:
        cols += [(gk * dk2[e]).astype(np.float64) * wgt for e in range(d)]
    else:
        cols.append(gl.astype(np.float64) * wgt)
    cols.append(np.where(diag, g.astype(np.float64), 0.0))
    out = []
    for i, terms in enumerate(cols):
        rec = _records(terms)
        if mutant == "drop1024":
            rec = rec[:1024]
        out.append(0.5 * _final(rec) * (noise if i == len(cols) - 1 else 1.0))
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------ inputs ----
def _alpha(n, q, seed):
    """Alternating signs down the rows: the sums cancel."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.5, 1.5, size=(n, q)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    return a.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _grad_problem(n, d, q, offset, seed=0):
    """x, a symmetric random ``Kinv`` (not an inverse: the kernel is a contraction) and alpha, float32-representable."""
    rng = np.random.RandomState(1000 * n + 10 * d + q + seed)
    x = cn.problem(n, d, n + d + seed, offset)
    k = rng.randn(n, n)
    kinv = ((k + k.T) / 2).astype(np.float32).astype(np.float64)
    return x, kinv, _alpha(n, q, n + q)


def _nan_upper(kinv):
    out = kinv.copy()
    out[np.triu_indices(len(kinv), 1)] = np.nan
    return out


def _ratio(got, ref, bnd):
    return float(np.max(np.abs(np.asarray(got, dtype=cn.LD) - ref) / bnd))


# ------------------------------------------------------------------------------------------------- clean arithmetic ----
@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_clean_arithmetic_is_inside_every_bound(dt, cov, capsys):
    ft, u = FT[dt], UNIT[dt]
    worst = dict(value=0.0, mean=0.0, grad=0.0)
    for d in DIMS:
        for offset in OFFSETS:
            x = cn.problem(96, d, 7 + d, offset)
            xs = np.vstack([x[:5], cn.problem(8, d, 70 + d, offset)[4:]])
            alpha, bias, pre = _alpha(96, 3, d), np.array([0.25, -1.5, 3.0]), _alpha(9, 3, 5)
            gx, gkinv, galpha = _grad_problem(129, d, 3, offset)
            for ell in ELLS:
                k, w = cn.value_terms(x, x, cov, ell, SF2)
                worst["value"] = max(worst["value"], _ratio(dev_value(x, x, cov, ell, SF2, ft), k, cn.bound(k, w, u)))
                for b, p in ((None, None), (bias, None), (bias, pre)):
                    m, wm = cn.mean_terms(x, alpha, xs, cov, ell, SF2, b, p)
                    got = dev_mean(x, alpha, xs, cov, ell, SF2, ft, b, p)
                    worst["mean"] = max(worst["mean"], _ratio(got, m, cn.bound(np.abs(m), wm, u)))
                for ard in (False, True):
                    ells = ARD_ELLS[:d] if ard else ell
                    xin = gx / ARD_ELLS[:d] if ard else gx
                    g, wg, sg = cn.lml_grad_terms(gx, _nan_upper(gkinv), galpha, 3, cov, ells, SF2, NOISE, ard)
                    got = dev_lml_grad(xin, gkinv, galpha, 3, cov, ell, SF2, NOISE, ard, ft)
                    assert np.isfinite(got).all()
                    worst["grad"] = max(worst["grad"], _ratio(got, g, cn.lml_grad_bound(g, wg, sg, u, 129)))
    _say(capsys, "clean restatement %s cov %d: worst err/bound value %.3f | mean %.3f | gradient %.3f"
         % (dt, cov, worst["value"], worst["mean"], worst["grad"]))
    assert max(worst.values()) <= 1.0


def test_the_planted_pairs_are_what_the_gpu_tests_assert():
    """The coincident pair gives exactly sf2, the far pair underflows for the RBF at ell <= 0.6, in both dtypes."""
    for dt in ("f32", "f64"):
        for d in DIMS:
            x = cn.problem(8, d, d, 1024.0)
            assert x[2, 0] - x[0, 0] == 2.0 ** -12 and np.all(np.abs(x[3] - x[0] - 30.0) < 1e-3) and np.all(x[1] == x[0])
            for cov in cn.COVS:
                k = dev_value(x, x, cov, 0.6, SF2, FT[dt])
                assert k[1, 0] == FT[dt](SF2) and np.isfinite(k).all()
            assert 0.0 <= dev_value(x, x, 0, 0.6, SF2, FT[dt])[3, 0] < 1e-30 * SF2


# --------------------------------------------------------------------------------------------------------- mutants ----
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_an_expanded_squared_distance_fails_at_the_offset(dt, capsys):
    """d2 = |a|^2 + |b|^2 - 2 a.b cancels about 2 x 10^6 down to O(1) beside 1024.  (The FP64 inputs get low bits here:
    squares and products of float32-representable numbers are exact in FP64.  Matern at d = 1 takes r = |a - b| and never
    looks at d2.)"""
    ft, u = FT[dt], UNIT[dt]
    for cov in cn.COVS:
        for d in (1, 3) if cov == 0 else (2, 3):
            x = cn.problem(96, d, 7 + d, 1024.0)
            if dt == "f64":
                x = x + np.random.RandomState(d).uniform(size=x.shape) * 2.0 ** -20
            k, w = cn.value_terms(x, x, cov, 0.6, SF2)
            ratio = _ratio(dev_value(x, x, cov, 0.6, SF2, ft, "expanded"), k, cn.bound(k, w, u))
            _say(capsys, "expanded d2 %s cov %d d %d: err/bound %.3g" % (dt, cov, d, ratio))
            assert ratio > 1.0


@pytest.mark.parametrize("cov", [1, 2, 3])
def test_a_smoothed_matern_radius_fails(cov, capsys):
    """r = sqrt(d2 + 1e-12): the coincident and the nearly coincident pair move by a relative O(c 1e-6) (nu = 1/2) or
    O(c^2 1e-12) (the smoother ones): outside the FP64 bound for every policy, outside the FP32 bound for nu = 1/2."""
    x = cn.problem(96, 3, 10, 0.0)
    k, w = cn.value_terms(x, x, cov, 2.0 ** -4, SF2)
    r64 = _ratio(dev_value(x, x, cov, 2.0 ** -4, SF2, np.float64, "eps"), k, cn.bound(k, w, UNIT["f64"]))
    r32 = _ratio(dev_value(x, x, cov, 2.0 ** -4, SF2, np.float32, "eps"), k, cn.bound(k, w, UNIT["f32"]))
    _say(capsys, "sqrt(d2 + eps) cov %d: err/bound f64 %.3g, f32 %.3g" % (cov, r64, r32))
    assert r64 > 1.0
    if cov == 1:
        assert r32 > 1.0


@pytest.mark.parametrize("cov", cn.COVS)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_one_far_entry_off_by_1e_4_passes_the_old_cap_and_fails_the_bound(dt, cov, capsys):
    ft, u = FT[dt], UNIT[dt]
    ell = 0.6 if cov == 0 else 2.0 ** -4                              # the Matern tails are long: a short length-scale
    x = cn.problem(96, 2, 9, 0.0)
    k, w = cn.value_terms(x, x, cov, ell, SF2)
    far = np.argwhere((k < 1e-10 * SF2) & (k > 1e-20 * SF2))          # 1e-10 x 1e-4 stays below the FP64 cap too
    assert len(far)
    i, j = far[0]
    got = dev_value(x, x, cov, ell, SF2, ft)
    got[i, j] *= ft(1.0 + 1e-4)
    old = float(np.max(np.abs(got.astype(np.float64) - np.asarray(k, dtype=np.float64))) / SF2)
    new = _ratio(got, k, cn.bound(k, w, u))
    _say(capsys, "far entry x (1 + 1e-4) %s cov %d: normwise %.2e (cap %.0e), err/bound %.3g" % (dt, cov, old, OLD_CAP[dt], new))
    assert old <= OLD_CAP[dt]
    assert new > 1.0


MUTANT_TILE = {"skip": 7, "twice": 4, "weight1": 11, "upper": 5}     # records of n = 300 (15): (3, 1), (2, 1), (4, 1), (2, 2)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("mutant", ["skip", "twice", "weight1", "upper", "alpha5"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_mutated_contraction_fails(dt, mutant, ard, capsys):
    n, d, q, cov, ell = 300, 2, 8, 2, 16.0
    x, kinv, alpha = _grad_problem(n, d, q, 0.0)
    ells = ARD_ELLS[:d] * 8 if ard else ell
    g, w, s = cn.lml_grad_terms(x, _nan_upper(kinv), alpha, q, cov, ells, SF2, NOISE, ard)
    bnd = cn.lml_grad_bound(g, w, s, UNIT[dt], n)
    xin = x / (ARD_ELLS[:d] * 8) if ard else x
    clean = _ratio(dev_lml_grad(xin, kinv, alpha, q, cov, ell, SF2, NOISE, ard, FT[dt]), g, bnd)
    bad = np.abs(dev_lml_grad(xin, kinv, alpha, q, cov, ell, SF2, NOISE, ard, FT[dt], mutant, MUTANT_TILE.get(mutant, 0)) - g) / bnd
    _say(capsys, "contraction %s %s ard=%d: clean %.3f, mutant err/bound %s" % (dt, mutant, ard, clean, np.array2string(
        np.asarray(bad, dtype=np.float64), precision=2)))
    assert clean <= 1.0
    assert float(np.max(bad)) > 1.0
    assert float(bad[0]) > 1.0                                      # the sf entry sees every one of them


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_dropping_the_records_past_1024_fails(dt, capsys):
    """n = 2945: 47 tile rows, 1128 records; the final kernel's thread t adds records t and t + 1024."""
    n, d, q, cov, ell = 2945, 2, 8, 2, 16.0
    assert len(cn.tile_ids(n)[0]) == 1128
    x, kinv, alpha = _grad_problem(n, d, q, 0.0)
    g, w, s = cn.lml_grad_terms(x, kinv, alpha, q, cov, ell, SF2, NOISE, False)
    bnd = cn.lml_grad_bound(g, w, s, UNIT[dt], n)
    clean = _ratio(dev_lml_grad(x, kinv, alpha, q, cov, ell, SF2, NOISE, False, FT[dt]), g, bnd)
    bad = np.abs(dev_lml_grad(x, kinv, alpha, q, cov, ell, SF2, NOISE, False, FT[dt], "drop1024") - g) / bnd
    _say(capsys, "contraction %s n = 2945: clean %.3f, records past 1024 dropped err/bound %s" % (dt, clean, np.array2string(
        np.asarray(bad, dtype=np.float64), precision=2)))
    assert clean <= 1.0
    assert float(np.min(bad)) > 1.0
