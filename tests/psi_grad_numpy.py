"""NumPy oracle of the gradients of the bound on uncertain inputs ("Gradients of the bound on uncertain
inputs"): the analytic derivatives of Psi1 and Psi2 contracted with a weight matrix, of the collapsed bound F and of the
KL term, parametrised by the float type ``ft`` like tests/psi_numpy.py, whose closed forms and linear algebra it reuses;
and the rounding bounds of the device kernels.  Test infrastructure only: nothing here is on the product path."""
import numpy as np

import psi_numpy as po
from psi_numpy import _f, ells


# -------------------------------------------------------------------------------------------- the psi contractions ----
def psi1_grad(mu, s, z, ell, sf, g1, ft=np.float64, bound=False, roundings=None):
    """The derivatives of sum g1 o Psi1: dict(dmu (n, d), ds (n, d), dz (m, d), sums (d + 1): d/dlog sf, d/dlog l_e).
    ``bound``: the values' rounding weights instead (:func:`grad_bound` documents them); ``roundings``: per unit of
    exponent, 3 d + 2 by default."""
    mu, s, z, g1 = _f(mu, ft), _f(s, ft), _f(z, ft), _f(g1, ft)
    n, d = mu.shape
    l2 = ells(ell, d, ft) ** 2
    p, t = po.psi1_parts(mu, s, z, ell, sf, ft)
    a = mu[:, None, :] - z[None, :, :]
    h = (1 / (l2 + s))[:, None, :]
    sh = (s / (l2 + s))[:, None, :]
    if not bound:
        w = (g1 * p)[:, :, None]
        return dict(dmu=(-w * a * h).sum(axis=1), ds=(w * (a * a * h * h - h) / 2).sum(axis=1), dz=(w * a * h).sum(axis=0),
                    sums=np.concatenate([[(g1 * p).sum()], (w * (sh + l2 * a * a * h * h)).sum(axis=(0, 1))]))
    m = z.shape[0]
    k, c = (3 * d + 2 if roundings is None else roundings), 2 * d + 20
    a = np.abs(a)
    base = (np.abs(g1) * p)[:, :, None]
    w = lambda terms: base * (terms + k * t[:, :, None] + c)                    # per addend: sum, exponent, the rest
    big = np.abs(g1)[:, :, None] * _f(sf, ft)                                   # an addend's factor of exp(.): the underflow floor
    fm, fs, fl = a * h, (a * a * h * h + h) / 2, sh + l2 * a * a * h * h
    one = np.ones_like(fm[:, :, :1])
    return dict(dmu=((w(m) * fm).sum(axis=1), (big * fm).sum(axis=1), m), ds=((w(m) * fs).sum(axis=1), (big * fs).sum(axis=1), m),
                dz=((w(n) * fm).sum(axis=0), (big * fm).sum(axis=0), n),
                sums=(np.concatenate([(w(n) * one).sum(axis=(0, 1)), (w(n) * fl).sum(axis=(0, 1))]),
                      np.concatenate([(big * one).sum(axis=(0, 1)), (big * fl).sum(axis=(0, 1))]), n * m))


def psi2_grad(mu, s, z, ell, sf, g2, ft=np.float64, bound=False, roundings=None):
    """The derivatives of sum_jk g2_jk Psi2_jk over ALL ordered pairs (g2 symmetric): dict(dmu, ds, dz, sums) as
    :func:`psi1_grad` has them, sums[0] = d/dlog sf = 2 sum g2 o Psi2.  ``bound``: the rounding weights instead
    (:func:`grad_bound`).  Per row i and pair, with a = mu_i - (z_j + z_k) / 2 and r = 1 / (l^2 + 2 s_i), the term
    w = g2_jk sf^2 exp(-delta_jk - t_ijk) is multiplied by -2 a r (dmu), 2 a^2 r^2 - r (ds), 2 [a r - (z_j - z_k) / (2 l^2)] (dz_j:
    both orders of the pair) and 2 s r + 2 l^2 a^2 r^2 + (z_j - z_k)^2 / (2 l^2) (log l); the parts that do not depend on the row are
    added after the loop over the rows."""
    mu, s, z, g2 = _f(mu, ft), _f(s, ft), _f(z, ft), _f(g2, ft)
    n, d = mu.shape
    m = z.shape[0]
    l2 = ells(ell, d, ft) ** 2
    delta = po.psi2_delta(z, ell, ft)
    zbar = (z[:, None, :] + z[None, :, :]) / 2
    zd = z[:, None, :] - z[None, :, :]
    scale = _f(sf, ft) ** 2 * np.exp(-delta)
    k, c = (3 * d + 2 if roundings is None else roundings), 2 * d + 20
    over = lambda w, x: np.tensordot(w, x, axes=([0, 1], [0, 1]))               # sum_jk w_jk x_jke
    dmu, ds = np.zeros((n, d), dtype=ft), np.zeros((n, d), dtype=ft)
    dz, sums = np.zeros((m, d), dtype=ft), np.zeros(d + 1, dtype=ft)
    if not bound:
        wsum = np.zeros((m, m), dtype=ft)
        for i, t in enumerate(po.psi2_rows(mu, s, z, ell, ft)):
            r = 1 / (l2 + 2 * s[i])
            w = g2 * scale * np.exp(-t)
            ar = (mu[i] - zbar) * r                                              # (m, m, d)
            saa, total = over(w, ar * ar), w.sum()
            dmu[i] = -2 * over(w, ar)
            ds[i] = 2 * saa - r * total
            dz += 2 * (w[:, :, None] * ar).sum(axis=1)
            sums[1:] += 2 * s[i] * r * total + 2 * l2 * saa
            wsum += w
        dz -= (wsum[:, :, None] * zd).sum(axis=1) / l2
        sums[0] = 2 * wsum.sum()
        sums[1:] += over(wsum, zd * zd) / (2 * l2)
        return dict(dmu=dmu, ds=ds, dz=dz, sums=sums)
    npairs, nz, nsum = m * (m + 1) // 2, n + 2 * m + 32, 16 * n + m * m
    big = np.abs(g2) * _f(sf, ft) ** 2 * 2                                        # an addend's factor of exp(.), both underflows
    fmu, fds, fdz, fsums = np.zeros_like(dmu), np.zeros_like(ds), np.zeros_like(dz), np.zeros_like(sums)     # the underflow floors
    wz, ws = np.zeros((m, m), dtype=ft), np.zeros((m, m), dtype=ft)
    for i, t in enumerate(po.psi2_rows(mu, s, z, ell, ft)):
        r = 1 / (l2 + 2 * s[i])
        sr = 2 * s[i] * r
        # |a| with the cancellation of (mu - z_j / 2) - z_k / 2 undone: the rounding of the first difference is relative to it
        hj = np.abs(mu[i] - z / 2)
        abr = (np.abs(mu[i] - zbar) + np.maximum(hj[:, None, :], hj[None, :, :])) * r
        abr2 = abr * abr
        base = np.abs(g2) * scale * np.exp(-t)
        per = k * (t + delta) + c
        wp, wq, wr = base * (npairs + per), base * (nz + per), base * (nsum + per)
        dmu[i], ds[i] = 2 * over(wp, abr), 2 * over(wp, abr2) + r * wp.sum()
        dz += 2 * (wq[:, :, None] * abr).sum(axis=1)
        sums[1:] += sr * wr.sum() + 2 * l2 * over(wr, abr2)
        fmu[i], fds[i] = 2 * over(big, abr), 2 * over(big, abr2) + r * big.sum()
        fdz += 2 * (big[:, :, None] * abr).sum(axis=1)
        fsums[1:] += sr * big.sum() + 2 * l2 * over(big, abr2)
        wz += wq
        ws += wr
    dz += (wz[:, :, None] * np.abs(zd)).sum(axis=1) / l2
    fdz += n * (big[:, :, None] * np.abs(zd)).sum(axis=1) / l2
    sums[0], fsums[0] = 2 * ws.sum(), 2 * n * big.sum()
    sums[1:] += over(ws, zd * zd) / (2 * l2)
    fsums[1:] += n * over(big, zd * zd) / (2 * l2)
    return dict(dmu=(dmu, fmu, npairs), ds=(ds, fds, npairs), dz=(dz, fdz, nz), sums=(sums, fsums, nsum))


def grad_bound(value, weights, u):
    """What a stored entry of the longdouble ``value`` may be off by in the format of unit roundoff ``u``:
    ``psi_numpy.bound``'s form over signed addends.  ``weights`` = (w, floor, terms) of :func:`psi1_grad` /
    :func:`psi2_grad` with ``bound=True``: w = sum over the entry's addends |g term factor| [terms + k (t + delta) + c].

    * k = 3 d + 2 roundings per unit of exponent, the count of ``psi_numpy.psi1_terms`` / ``psi2_terms``: the kernels form
      the exponent with the same operations (c0 and r_e or h_e rounded once; a difference, a square and a multiply-add per
      dimension).
    * c = 2 d + 20: the exponential, the weight g sf^2 exp(-delta) (three products and delta's d multiply-adds) and the
      stored value, which 2 d + 12 covers as it does for Psi2; and eight more for the factor: q = a r (the difference's two
      roundings, r's own, the product), p q, the multiply-add with q, and the final scaling and subtraction.
    * terms: the addends of the entry's longest chain of additions (the pairs of a row; the rows and tiles of a point).
    * factor: in its cancellation-free magnitude -- every part in absolute value, and |a| taken as |a| + |mu - z_j / 2|
      for Psi2, whose a = (mu - z_j / 2) - z_k / 2 carries the rounding of its first difference.
    * floor: an exponential (or its product with exp(-delta)) that underflows is off by at most the smallest normal
      number: ``floor`` is the sum of the addends' factors of it, and terms + 2 more cover the sums' own underflow."""
    w, floor, terms = weights
    tiny = po.tiny(u)
    return np.asarray(u * w + u * np.abs(value) + tiny * (floor + terms + 2), dtype=np.float64)


# ------------------------------------------------------------------------------------------------- the bound's gradient ----
def solve_upper_t(l, b):
    """L^-T b by back substitution."""
    b = np.array(b, copy=True)
    x = np.zeros_like(b)
    for i in range(l.shape[0] - 1, -1, -1):
        x[i] = (b[i] - l[i + 1:, i] @ x[i + 1:]) / l[i, i]
    return x


def kuu_grad(z, ell, sf, eps, g, ft=np.float64):
    """The derivatives of sum G o (K(Z, Z) + eps sf I) for a symmetric G: (d/dlog sf, d/dlog l_e (d,), dZ (m, d))."""
    z, g = _f(z, ft), _f(g, ft)
    m, d = z.shape
    l2 = ells(ell, d, ft) ** 2
    k = po.kern(z, z, ell, sf, ft)
    zd = z[:, None, :] - z[None, :, :]
    w = (g * k)[:, :, None]
    return (g * k).sum() + _f(eps, ft) * _f(sf, ft) * np.trace(g), (w * zd * zd / l2).sum(axis=(0, 1)), (-2 * w * zd / l2).sum(axis=1)


def kl_parts(mu, s, prior_mean=None, prior_var=None, ft=np.float64):
    """(KL, dKL/dmu, dKL/ds) of q(x) = N(mu, diag s) against N(prior_mean, diag prior_var) over the entries with s > 0 (None:
    N(0, 1)); the gradients are zero at the entries with s = 0."""
    mu, s = _f(mu, ft), _f(s, ft)
    pm = np.zeros_like(mu) if prior_mean is None else np.broadcast_to(_f(prior_mean, ft), mu.shape)
    pv = np.ones_like(mu) if prior_var is None else np.broadcast_to(_f(prior_var, ft), mu.shape)
    pos = s > 0
    safe = np.where(pos, s, _f(1, ft))
    zero = _f(0, ft)
    kl = np.where(pos, (safe + (mu - pm) ** 2) / pv - 1 - np.log(safe / pv), zero).sum() / 2
    return kl, np.where(pos, (mu - pm) / pv, zero), np.where(pos, (1 / pv - 1 / safe) / 2, zero)


def bound_grad(mu, s, z, y, ell, sf, noise, eps=1e-6, ft=np.float64):
    """(F, dict(dsf, dl (d,), dnoise, dz, dmu, ds)): the collapsed bound of ``psi_numpy.Model`` and its analytic gradient
    w.r.t. log sf, log l_e, log noise, Z, mu and s ((n, d): a shared variance is broadcast first).  With P = Psi2,
    b = Psi1^T Y, A = K_uu + P / s2 = L_u B L_u^T, u = L_B^-T gamma and v = L_u^-T u:
        dF/dPsi1 = Y v^T / s2            dF/dP = L_u^-T [q / (2 s2) (I - B^-1) - u u^T / (2 s2)] L_u^-1
        dF/dK_uu = -q/2 (A^-1 - K_uu^-1) - 1/2 v v^T - q / (2 s2) K_uu^-1 P K_uu^-1
        dF/dlog s2 = -n q / 2 + q/2 (m - tr B^-1) + |Y|^2 / (2 s2) - 1/2 |gamma|^2 - 1/2 |u|^2 + q (psi0 - tr T) / (2 s2)
    and psi0 = n sf."""
    mdl = po.Model(mu, s, z, y, ell, sf, noise, eps, ft)
    mu, z, y, s = mdl.mu, mdl.z, _f(y, ft), np.array(mdl.s)
    n, d = mu.shape
    m, q = z.shape[0], y.shape[1]
    sf_, s2 = mdl.sf, mdl.noise
    eye = np.eye(m, dtype=ft)
    lu_inv = po.solve_lower(mdl.lu, eye)                                         # L_u^-1
    lb_inv = po.solve_lower(mdl.lb, eye)
    binv = lb_inv.T @ lb_inv
    u = solve_upper_t(mdl.lb, mdl.gamma)                                          # (m, q)
    v = lu_inv.T @ u
    g1 = y @ v.T / s2
    inner = (q / (2 * s2)) * (eye - binv) - (u @ u.T) / (2 * s2)
    g2 = lu_inv.T @ inner @ lu_inv
    g2 = (g2 + g2.T) / 2
    p2 = po.psi2(mu, s, z, ell, sf_, ft)
    kinv = lu_inv.T @ lu_inv
    ainv = lu_inv.T @ binv @ lu_inv
    guu = -(q / _f(2, ft)) * (ainv - kinv) - (v @ v.T) / 2 - (q / (2 * s2)) * (kinv @ p2 @ kinv)
    guu = (guu + guu.T) / 2
    t = lu_inv @ p2 @ lu_inv.T
    a1, a2 = psi1_grad(mu, s, z, ell, sf_, g1, ft), psi2_grad(mu, s, z, ell, sf_, g2, ft)
    ksf, kl_, kz = kuu_grad(z, ell, sf_, eps, guu, ft)
    dnoise = (-_f(n * q, ft) / 2 + _f(q, ft) / 2 * (m - np.trace(binv)) + (y ** 2).sum() / (2 * s2) - (mdl.gamma ** 2).sum() / 2
              - (u ** 2).sum() / 2 + q * (n * sf_ - np.trace(t)) / (2 * s2))
    grad = dict(dsf=a1['sums'][0] + a2['sums'][0] + ksf - q * n * sf_ / (2 * s2), dl=a1['sums'][1:] + a2['sums'][1:] + kl_,
                dnoise=dnoise, dz=a1['dz'] + a2['dz'] + kz, dmu=a1['dmu'] + a2['dmu'], ds=a1['ds'] + a2['ds'])
    return mdl.bound, grad


def elbo_grad(mu, s, z, y, ell, sf, noise, eps=1e-6, prior_mean=None, prior_var=None, ft=np.float64):
    """(F - KL, gradient): :func:`bound_grad` with the KL term's gradient taken from dmu and ds."""
    f, g = bound_grad(mu, s, z, y, ell, sf, noise, eps, ft)
    n, d = np.shape(mu)
    kl, kmu, ks = kl_parts(mu, np.broadcast_to(_f(s, ft), (n, d)), prior_mean, prior_var, ft)
    g = dict(g, dmu=g['dmu'] - kmu, ds=g['ds'] - ks)
    return f - kl, g


# ------------------------------------------------------------------------------------------------ the scratch sizes ----
def _slices_for(n, units, target=2048, min_slice=64, align=16):
    """(S, slice length) by the slice rule of include/cimrgp_psi.h for ``units`` workgroups per slice."""
    s0 = max(1, min(target // units, -(-n // min_slice)))
    length = -(-(-(-n // s0)) // align) * align
    return -(-n // length), length


def _r16(b):
    return -(-b // 16) * 16


def psi1_grad_scratch_bytes(esz, n, m, d):
    """cimrgp_psi1_grad_scratch_bytes: S m d partial sums of dz and S ceil(m / 64) (d + 1) float64 partial sums."""
    cbs = -(-m // 64)
    s = _slices_for(n, cbs)[0]
    return _r16(s * m * d * esz) + _r16(s * cbs * (d + 1) * 8)


def psi2_grad_scratch_bytes(esz, n, m, d, row_wgs=1024):
    """cimrgp_psi2_grad_scratch_bytes: the counts, the rows' 3 d + 1 constants, the P shares of (dmu, ds), and per (slice, tile)
    of the pairs pass 2 E d partial sums of dz and d + 1 float64 partial sums."""
    t64 = -(-m // 64)
    shares = max(1, min(t64 * (t64 + 1) // 2, row_wgs // -(-n // 256)))
    edge = 64 if d <= 2 else 32
    t = -(-m // edge)
    tiles = t * (t + 1) // 2
    units = _slices_for(n, tiles)[0] * tiles
    return (_r16(-(-n // 256) * 8) + _r16(n * (3 * d + 1) * esz) + _r16(shares * n * 2 * d * esz) + _r16(units * 2 * edge * d * esz)
            + _r16(units * (d + 1) * 8))
