"""NumPy oracle of the predictive variance at uncertain test inputs ("Predictive variance at uncertain test
inputs"): a row's own Psi2 contracted with two weights (include/cimrgp_psi_rows.h) with the rounding bound of the device
kernel, the moments of ``psi_numpy.Model`` at Gaussian test inputs, their Gauss-Hermite evaluation by the law of total
variance (an independent check of the closed form), and the header's grouping and scratch size restated.  Parametrised by
the float type ``ft`` like tests/psi_numpy.py, whose closed forms and linear algebra it reuses.  Test infrastructure only:
nothing here is on the product path."""
import numpy as np

import psi_grad_numpy as pg
import psi_numpy as po
from psi_numpy import _f

GROUPS = 16                                    # CIMRGP_PSI_ROWS_GROUPS


# ------------------------------------------------------------------------------------------------ the contraction ----
def rows_quad(mu, s, z, ell, sf, c, a, ft=np.float64, bound=False, roundings=None):
    """dict(tr (n,), quad (n, q)): tr_i = sum_jk c_jk Psi2_i[j][k] and quad_ic = a_c^T Psi2_i a_c over the full square, with
    Psi2_i[j][k] = sf^2 exp(-delta_jk - t_ijk) the row's own term (``psi_numpy.psi2_rows``); ``c`` symmetric (m, m), ``a``
    (m, q).  ``bound``: the values' rounding weights instead, (w, floor, terms) per key for ``psi_grad_numpy.grad_bound``,
    counted as that function counts them:

    * k = 3 d + 2 roundings per unit of the exponent t + delta (``roundings``): the kernel forms the exponent with the
      operations of cimrgp_psi2 (c0 and r_e rounded once; a difference, a square and a multiply-add per dimension), delta
      likewise from the halved points.
    * c = 2 d + 16 for the rest of an addend: the two exponentials, sf^2 and its product with exp(-delta) and delta's d
      multiply-adds, which 2 d + 12 covers as it does for Psi2; and four more for the products with the weight -- c_jk
      (tr), or exp's weight times the row's exponential, a_kc and a_jc (quad).
    * terms: one rounding per addend of the longest chain of additions, the m (m + 1) / 2 pairs of a row and the GROUPS
      subtotals.
    * every addend in absolute value, since c and a are signed: w = sum_jk |weight_jk| term_ijk [terms + k (t + delta) + c].
    * floor: an exponential that underflows is off by at most the smallest normal number; ``floor`` is the sum of the
      addends' factors of it (both exponentials)."""
    mu, s, z, c, a = _f(mu, ft), _f(s, ft), _f(z, ft), _f(c, ft), _f(a, ft)
    n, d = mu.shape
    m, q = a.shape
    delta = po.psi2_delta(z, ell, ft)
    scale = _f(sf, ft) ** 2 * np.exp(-delta)
    tr, quad = np.zeros(n, dtype=ft), np.zeros((n, q), dtype=ft)
    if not bound:
        for i, t in enumerate(po.psi2_rows(mu, s, z, ell, ft)):
            p = scale * np.exp(-t)
            tr[i] = (c * p).sum()
            quad[i] = ((p @ a) * a).sum(axis=0)
        return dict(tr=tr, quad=quad)
    k, rest, terms = (3 * d + 2 if roundings is None else roundings), 2 * d + 16, m * (m + 1) // 2 + GROUPS
    ac, aa = np.abs(c), np.abs(a)
    big = 2 * _f(sf, ft) ** 2
    for i, t in enumerate(po.psi2_rows(mu, s, z, ell, ft)):
        w = scale * np.exp(-t) * (terms + k * (t + delta) + rest)
        tr[i] = (ac * w).sum()
        quad[i] = ((w @ aa) * aa).sum(axis=0)
    ftr = np.full(n, big * ac.sum(), dtype=ft)
    fquad = np.broadcast_to(big * aa.sum(axis=0) ** 2, (n, q)).astype(ft)
    return dict(tr=(tr, ftr, terms), quad=(quad, fquad, terms))


# --------------------------------------------------------------------------------------------------- the moments ----
def weights(model):
    """(C, a) of a ``psi_numpy.Model``: C = L_u^-T (I - B^-1) L_u^-1 (symmetrised) and a = L_u^-T L_B^-T gamma."""
    ft = model.ft
    m = model.z.shape[0]
    eye = np.eye(m, dtype=ft)
    lu_inv, lb_inv = po.solve_lower(model.lu, eye), po.solve_lower(model.lb, eye)
    c = lu_inv.T @ (eye - lb_inv.T @ lb_inv) @ lu_inv
    return (c + c.T) / 2, lu_inv.T @ pg.solve_upper_t(model.lb, model.gamma)


def moments(model, xs, xs_var, include_noise=False):
    """(mean (ns, q), var (ns, q)) of the model's prediction at x*_i ~ N(xs_i, diag xs_var_i) (a scalar or a (d,) vector is
    broadcast): var_ic = sf - sum C o Psi2*_i + a_c^T Psi2*_i a_c - mean_ic^2 (+ noise)."""
    ft = model.ft
    xs = _f(xs, ft)
    sv = np.broadcast_to(_f(xs_var, ft), xs.shape)
    c, a = weights(model)
    mean = model.predict_uncertain(xs, sv)
    r = rows_quad(xs, sv, model.z, model.ell, model.sf, c, a, ft)
    var = (model.sf - r['tr'])[:, None] + (r['quad'] - mean ** 2)
    return mean, var + model.noise if include_noise else var


def moments_gauss_hermite(model, xs, xs_var, nodes=60):
    """The same moments by a nodes^d Gauss-Hermite rule over ``model.predict`` (d <= 2), by the law of total variance:
    mean = E mean(x*), var = E var(x*) + E mean(x*)^2 - (E mean(x*))^2."""
    ft = model.ft
    xs = _f(xs, ft)
    sv = np.broadcast_to(_f(xs_var, ft), xs.shape)
    ns, d = xs.shape
    assert d <= 2
    t, w = np.polynomial.hermite.hermgauss(nodes)
    t, w = _f(t, ft), _f(w, ft) / np.sqrt(_f(np.pi, ft))
    pts = np.stack([g.ravel() for g in np.meshgrid(*([t] * d), indexing="ij")], axis=1)
    wts = np.prod(np.stack(np.meshgrid(*([w] * d), indexing="ij"), axis=0), axis=0).ravel()
    wts = wts / wts.sum()
    mean, var = [], []
    for i in range(ns):
        mk, vk = model.predict(xs[i] + np.sqrt(2 * sv[i]) * pts)
        em = wts @ mk
        mean.append(em)
        var.append(wts @ vk + (wts @ (mk - em) ** 2))
    return np.array(mean), np.array(var)


# ------------------------------------------------------------------------------------------------ the scratch size ----
def group_rule(m, tile=64, groups=GROUPS):
    """(G, tiles per group, tiles) by the rule of include/cimrgp_psi_rows.h: a function of m alone."""
    t = -(-m // tile)
    tiles = t * (t + 1) // 2
    per = -(-tiles // groups)
    return -(-tiles // per), per, tiles


def scratch_bytes(esz, n, m, d, q):
    """cimrgp_psi2_rows_quad_scratch_bytes: the counts, the rows' 2 d + 1 constants and the G subtotals of every row's 1 + q
    sums, each part a multiple of 16 bytes."""
    r16 = lambda b: -(-b // 16) * 16
    return r16(-(-n // 256) * 8) + r16(n * (2 * d + 1) * esz) + r16(group_rule(m)[0] * n * (1 + q) * esz)
