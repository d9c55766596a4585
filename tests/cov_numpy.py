"""NumPy oracle of the dense covariance kernels (gram.hip, misc.hip, common.hpp's Cov<COV>): the value of the four policies
(cov = 0 RBF, 1 .. 3 Matern 1/2, 3/2, 5/2), the fused predictive mean and the contraction of the log marginal likelihood's
gradient, all in numpy.longdouble, each with the weight of a bound that counts the roundings of the device kernel (the
form of tests/psi_numpy.py: an entry stored at unit roundoff u may be off by u w + u |value| + the underflow floor).  Test
infrastructure only: nothing here is on the product path.

The counting, from the source.  Write t = |c| d2 for the RBF (c = -1 / (2 l^2)) and t = c r for the Matern policies
(c = sqrt(2 nu) / l), d2 = sum_k (a_k - b_k)^2 added in dimension order in the dtype (gram_lanes).

  RBF     d2 takes three roundings per dimension (the difference, its square, the add), all relative to a part of d2; the
          scale c is rounded once on the host and its product with d2 once: the exponent is off by at most (3 d + 2) u t.
          Then the exponential, the product with sf2 and (on the diagonal) diag_add: 2 d + 12 covers them with the margin
          the psi bounds have.  w = k [(3 d + 2) t + 2 d + 12]: psi_numpy.psi1_terms at s = 0.
  Matern  r = sqrt(d2) halves d2's relative error (1.5 d) and adds the root's rounding; c and c r add two more:
          t is off by (1.5 d + 3) u t.  (d = 1 takes r = |a - b|: fewer roundings, the same bound.)  k = sf2 p(t) exp(-t)
          moves by |dk/dt| dt <= k (t + t p'(t) / p(t)) dt / t, and the polynomial's own roundings (at most four), the
          exponential and the two products are inside 2 d + 12.  w = k [(1.5 d + 3)(t + t p'(t) / p(t)) + 2 d + 12].

The restatement of the kernels' operation order in NumPy (tests/test_cov_host.py) reaches, over d in {1, 2, 3, 8}, ell in
{0.6, 2^-4, 16}, the inputs of :func:`problem` with and without the offset 1024, at most these fractions of the bounds:
"""
# worst err / bound of the clean restatement, as printed by tests/test_cov_host.py (value | mean | gradient):
#   f32 cov 0: 0.578 | 0.144 | 0.023      f64 cov 0: 0.320 | 0.129 | 0.017
#   f32 cov 1: 0.363 | 0.137 | 0.025      f64 cov 1: 0.329 | 0.143 | 0.017
#   f32 cov 2: 0.471 | 0.129 | 0.013      f64 cov 2: 0.375 | 0.132 | 0.020
#   f32 cov 3: 0.419 | 0.154 | 0.011      f64 cov 3: 0.386 | 0.184 | 0.017
# (the gradient's bound is a worst case over n (n + 1) / 2 signed terms that mostly cancel; the mutants of
# tests/test_cov_host.py -- one 64-tile of 15 skipped, doubled or mis-weighted -- still exceed it 40 to 10^11 times)
import numpy as np

from psi_numpy import bound, tiny  # noqa: F401  (re-exported: the tests take both from here)

LD = np.longdouble
TILE = 64                       # k_lml_grad_tiles: LG_T
FINAL_THREADS = 1024            # k_lml_grad_final
PM_PH = 32                      # k_predict_mean: partial sums per test point
NU2 = {1: 1, 2: 3, 3: 5}        # 2 nu of the Matern policies
COVS = (0, 1, 2, 3)


def _f(a, ft=LD):
    return np.asarray(a, dtype=ft)


def problem(n, d, seed, offset=0.0):
    """(n, d) inputs uniform in [-2, 2] (+ ``offset``), exactly representable in float32 (returned as float64), so that both
    dtypes see the same problem and share one reference.  Planted, as far as n allows: row 1 = row 0 (a coincident pair),
    row 2 = row 0 + 2^-12 in coordinate 0 (nearly coincident: representable beside 1024 too, where float32's spacing is
    2^-13), row 3 = row 0 + 30 in every coordinate (a far pair)."""
    rng = np.random.RandomState(seed)
    x = (rng.uniform(-2.0, 2.0, size=(n, d)) + offset).astype(np.float32)
    if n > 1:
        x[1] = x[0]
    if n > 2:
        x[2] = x[0]
        x[2, 0] = x[0, 0] + np.float32(2.0 ** -12)
    if n > 3:
        x[3] = x[0] + np.float32(30.0)
    return x.astype(np.float64)


# ------------------------------------------------------------------------------------------------- one pair of points ----
def _pair(dfs, cov, ell, sf2):
    """Everything the bounds need of pairs with coordinate differences ``dfs`` (a list of d equal-shaped longdouble arrays):
    a dict with d2, t, r, c, the value k and its weight wk, the isotropic length-scale factor dl = dk / dlog l with weight
    wdl, and the per-dimension factor a (dk / dlog l_e = a df_e^2 at equal length-scales) with weight wa."""
    d = len(dfs)
    sf2, ell = LD(sf2), LD(ell)
    d2 = np.zeros_like(dfs[0])
    for df in dfs:
        d2 = d2 + df * df
    tail = 2 * d + 12
    if cov == 0:
        t = d2 / (2 * ell * ell)
        k = sf2 * np.exp(-t)
        wk = k * ((3 * d + 2) * t + tail)
        # dl = k d2 / l^2 is formed by the kernel from k, d2 and 1 / l^2: its factor is k (the products are counted there)
        return dict(d2=d2, t=t, k=k, wk=wk, dl=k, wdl=wk, a=k, wa=wk, lmul=d2 / (ell * ell))
    c = np.sqrt(LD(NU2[cov])) / ell
    r = np.sqrt(d2)
    t = c * r
    v = np.exp(-t)
    rt = 1.5 * d + 3
    if cov == 1:
        p, tdp, dl = 1.0, 0.0, sf2 * t * v
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(r > 0, sf2 * c * v / np.where(r > 0, r, 1), LD(0))       # the header's convention: 0 at r = 0
        ndl = 1
    elif cov == 2:
        p, tdp, dl, a = 1 + t, t, sf2 * t * t * v, c * c * sf2 * v
        ndl = 2
    else:
        p, tdp, dl, a = 1 + t + t * t / 3, t * (1 + 2 * t / 3), sf2 * t * t * (1 + t) * v / 3, c * c * sf2 * (1 + t) * v / 3
        ndl = 3
    k = sf2 * p * v
    wk = k * (rt * (t + tdp / p) + tail)
    # |d log dl / d log t| <= ndl + t (ndl = the power of t in front, + t / (1 + t) < 1 for nu = 5/2), |d log a / d log t| <= 1 + t
    wdl = dl * (rt * (ndl + t) + tail)
    wa = a * (rt * (1 + t) + tail)
    return dict(d2=d2, t=t, k=k, wk=wk, dl=dl, wdl=wdl, a=a, wa=wa, lmul=LD(1))


def _diffs(xa, xb):
    xa, xb = _f(xa), _f(xb)
    return [xa[..., :, None, e] - xb[..., None, :, e] for e in range(xa.shape[-1])]


def value_terms(xa, xb, cov, ell, sf2):
    """(k, w) of k(xa_i, xb_j) in longdouble: a stored entry may be off by u w + u k + 3 tiny(u) (:func:`bound`)."""
    p = _pair(_diffs(xa, xb), cov, ell, sf2)
    return p["k"], p["wk"]


def mean_terms(x, alpha, xs, cov, ell, sf2, bias=None, prefill=None):
    """(mean, w) of cimrgp_cov_predict_mean, (ns, q) each.  k_predict_mean: a lane adds its ceil(n / 32) products in the
    dtype (one rounding for the product, one per add: the j-th term sees at most ceil(n / 32) + 1 of them), then the 32
    partial sums and the bias are added in order (33 more): sum_j |alpha_j| (w_j + k_j (ceil(n / 32) + 34)).  The issue's
    formula has no term for the bias; the source adds it first, so it rides through the 32 adds: + 33 |bias|.  An
    accumulating call adds the old value once more: one rounding on |prefill| + |sum| (the stored value's own u |mean| is
    :func:`bound`'s)."""
    k, wk = value_terms(xs, x, cov, ell, sf2)
    alpha = _f(alpha)
    n = alpha.shape[0]
    steps = -(-n // PM_PH) + PM_PH + 2
    mean = k @ alpha
    w = wk @ np.abs(alpha) + steps * (k @ np.abs(alpha))
    if bias is not None:
        mean = mean + _f(bias)
        w = w + (PM_PH + 1) * np.abs(_f(bias))
    if prefill is not None:
        w = w + np.abs(_f(prefill)) + np.abs(mean)
        mean = mean + _f(prefill)
    return mean, w


# ------------------------------------------------------------------------------------------- the gradient contraction ----
def tile_ids(n, tile=TILE):
    """(ti, tj) of the tile records of the lower triangle in the kernel's order: id = ti (ti + 1) / 2 + tj, tj <= ti."""
    tm = -(-n // tile)
    ti = np.repeat(np.arange(tm), np.arange(1, tm + 1))
    tj = np.concatenate([np.arange(i + 1) for i in range(tm)])
    return ti, tj


def tile_layout(n, tile=TILE):
    """The pairs of the records as (T, tile, tile) arrays: row and column indices (clamped to n - 1 where they lie outside)
    and wgt = 1 on the diagonal, 2 strictly below it, 0 elsewhere (outside the matrix, above the diagonal)."""
    ti, tj = tile_ids(n, tile)
    gr = (ti[:, None] * tile + np.arange(tile))[:, :, None]
    gc = (tj[:, None] * tile + np.arange(tile))[:, None, :]
    live = (gr < n) & (gc < n) & (gc <= gr)
    wgt = np.where(live, np.where(gr == gc, 1, 2), 0)
    return np.minimum(gr, n - 1), np.minimum(gc, n - 1), wgt


def sum_steps(n):
    """FP64 additions a term of k_lml_grad_tiles / k_lml_grad_final can pass through: 16 terms per thread, 6 butterfly steps,
    sum4's 3, ceil(records / 1024) records per thread of the final kernel, then block_sum's 6 + 4 ( = 10 in the issue's count)
    and the 16 waves."""
    records = len(tile_ids(n)[0])
    return 16 + 6 + 3 + -(-records // FINAL_THREADS) + 10 + 16


def lml_grad_terms(x, kinv, alpha, q, cov, ell, sf2, noise, ard):
    """(g, w, s): the 3 (or, ``ard``, d + 2) entries [sf | l or l_1 .. l_d | noise] of cimrgp_cov_lml_grad[_ard] in longdouble
    from the LOWER triangle of ``kinv`` (what lies above the diagonal is not looked at), the weight w of the roundings made
    in the dtype and s = the sum of the |terms| that the FP64 sums run over; :func:`lml_grad_bound` makes the bound.
    ``ard``: ``ell`` holds the d length-scales and the inputs the device gets are x / ell (choose powers of two).

    Per pair (i >= j; twice off the diagonal) and entry the kernel adds g F M with
      g = sum_c alpha_ic alpha_jc - q Kinv_ij      (q products, q adds, q Kinv, the difference: q + 2 roundings on
                                                    A = sum_c |alpha_ic alpha_jc| + q |Kinv_ij|)
      F = the kernel factor with its own weight    (k for sf; RBF: k again for l and l_e; Matern: dk/dlog l, or a of the
                                                    header's r = 0 convention)
      M = 1 | d2 / l^2 (RBF, l) | df_e^2 (ARD)     (RBF l: d2's 3 d, 1 / l^2 and the two products: 3 d + 3; ARD: the
                                                    difference, its square and the product: 3; one more for g F)
    so the term is off by u [(q + 2) A |F| + |g| w_F + |g F| (roundings of M + 2)] M."""
    x, alpha = _f(x), _f(alpha)
    n, d = x.shape
    if ard:
        x, ell_iso = x / _f(ell), 1.0
    else:
        ell_iso = ell
    ri, ci, wgt = tile_layout(n)
    kin = np.where(wgt > 0, _f(kinv)[ri, ci], LD(0))
    xa, xb = x[ri[:, :, 0]], x[ci[:, 0, :]]
    dfs = [xa[:, :, None, e] - xb[:, None, :, e] for e in range(d)]
    p = _pair(dfs, cov, ell_iso, sf2)
    aa, ab = alpha[ri[:, :, 0]], alpha[ci[:, 0, :]]
    aat = np.einsum("tic,tjc->tij", aa, ab)
    big_a = np.einsum("tic,tjc->tij", np.abs(aa), np.abs(ab)) + q * np.abs(kin)
    g = aat - q * kin
    wl = _f(wgt)

    def entry(f, wf, m, roundings):
        term = g * f * m
        w = ((q + 2) * big_a * np.abs(f) + np.abs(g) * wf + np.abs(g * f) * (roundings + 2)) * np.abs(m)
        return (wl * term).sum(), (wl * w).sum(), (wl * np.abs(term)).sum()

    out = [entry(p["k"], p["wk"], LD(1), 0)]
    if ard:
        out += [entry(p["a"], p["wa"], dfs[e] * dfs[e], 3) for e in range(d)]
    elif cov == 0:
        out.append(entry(p["k"], p["wk"], p["lmul"], 3 * d + 3))
    else:
        out.append(entry(p["dl"], p["wdl"], LD(1), 0))
    diag = wgt == 1
    out.append((np.where(diag, g, 0).sum() * LD(noise), ((q + 2) * np.where(diag, big_a, 0)).sum() * LD(noise),
                np.abs(np.where(diag, g, 0)).sum() * LD(noise)))
    g_, w_, s_ = (np.array([o[i] for o in out], dtype=LD) / 2 for i in range(3))
    return g_, w_, s_


def lml_grad_bound(g, w, s, u, n):
    """What an output (a double) may be off by: the dtype's roundings of the terms (u w), the FP64 sums (2^-53 per step on
    s), the final product's rounding, and the dtype's underflow floor once per pair."""
    return np.asarray(u * w + 2.0 ** -53 * (sum_steps(n) * s + 2 * np.abs(g)) + n * (n + 1) * tiny(u), dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the small reductions ----
def reduction_steps(count):
    """Additions a term can pass through in a one-workgroup reduction over ``count`` elements (block_sum, reduce.hpp):
    ceil(count / 1024) per thread, 6 butterfly steps, 16 waves, and the roundings around the sum: ceil(count / 1024) + 24."""
    return -(-count // FINAL_THREADS) + 24


def logdet_terms(diag):
    """(sum_i log l_ii, sum_i |log l_ii|) in longdouble."""
    lg = np.log(_f(diag))
    return lg.sum(), np.abs(lg).sum()


def block_stats_terms(y):
    """(stats, s) of cimrgp_block_stats in longdouble for y (n, q), no fbar: the q column means and the pooled population
    variance about them, and per entry the sum of |terms| (|y_ic| / n; (y_ic - mean_c)^2 / (n q))."""
    y = _f(y)
    n, q = y.shape
    mean = y.sum(axis=0) / n
    r2 = (y - mean) ** 2
    return np.r_[mean, r2.sum() / (n * q)], np.r_[np.abs(y).sum(axis=0) / n, r2.sum() / (n * q)]
