"""NumPy oracle of the sparse GP on uncertain inputs ("Sparse GP regression on uncertain inputs"): the dense
psi statistics of the RBF covariance under x_i ~ N(mu_i, diag s_i), parametrised by the float type ``ft`` (numpy.float64 or
numpy.longdouble), their Gauss-Hermite evaluation for d <= 2 (an independent check of the closed forms), the shared-variance
factorisation, the rounding bounds of the device kernels, and the collapsed bound with its prediction.  Test
infrastructure only: nothing here is on the product path.  numpy.linalg has no longdouble, so the factorisation and the
triangular solves are written out."""
import numpy as np


def _f(a, ft):
    return np.asarray(a, dtype=ft)


def ells(ell, d, ft=np.float64):
    """(d,) length-scales from a scalar or a vector."""
    e = _f(ell, ft)
    return np.full(d, e, dtype=ft) if e.ndim == 0 else e


def kern(xa, xb, ell, sf, ft=np.float64):
    xa, xb = _f(xa, ft), _f(xb, ft)
    l = ells(ell, xa.shape[1], ft)
    d2 = (((xa[:, None, :] - xb[None, :, :]) / l) ** 2).sum(axis=2)
    return _f(sf, ft) * np.exp(-d2 / 2)


def psi1_parts(mu, s, z, ell, sf, ft=np.float64):
    """(Psi1, t): Psi1 = sf exp(-t), t_ij = 1/2 sum_e [log1p(s_ie / l_e^2) + (mu_ie - z_je)^2 / (l_e^2 + s_ie)]."""
    mu, s, z = _f(mu, ft), _f(s, ft), _f(z, ft)
    l2 = ells(ell, mu.shape[1], ft) ** 2
    t = (np.log1p(s / l2).sum(axis=1)[:, None] + ((mu[:, None, :] - z[None, :, :]) ** 2 / (l2 + s)[:, None, :]).sum(axis=2)) / 2
    return _f(sf, ft) * np.exp(-t), t


def psi1(mu, s, z, ell, sf, ft=np.float64):
    return psi1_parts(mu, s, z, ell, sf, ft)[0]


def psi2_delta(z, ell, ft=np.float64):
    """delta_jk = sum_e (z_je - z_ke)^2 / (4 l_e^2)."""
    z = _f(z, ft)
    l2 = ells(ell, z.shape[1], ft) ** 2
    return ((z[:, None, :] - z[None, :, :]) ** 2 / (4 * l2)).sum(axis=2)


def psi2_rows(mu, s, z, ell, ft=np.float64):
    """Yields per row i (an m x m matrix): t_ijk = 1/2 sum_e log1p(2 s_ie / l_e^2) + sum_e (mu_ie - (z_je + z_ke) / 2)^2 /
    (l_e^2 + 2 s_ie), the row exponent; a row's term of Psi2 is sf^2 exp(-delta_jk - t_ijk)."""
    mu, s, z = _f(mu, ft), _f(s, ft), _f(z, ft)
    l2 = ells(ell, mu.shape[1], ft) ** 2
    zbar = (z[:, None, :] + z[None, :, :]) / 2
    for i in range(mu.shape[0]):
        yield np.log1p(2 * s[i] / l2).sum() / 2 + ((mu[i] - zbar) ** 2 / (l2 + 2 * s[i])).sum(axis=2)


def psi2(mu, s, z, ell, sf, ft=np.float64):
    delta = psi2_delta(z, ell, ft)
    acc = np.zeros(delta.shape, dtype=ft)
    for t in psi2_rows(mu, s, z, ell, ft):
        acc += np.exp(-t)
    return _f(sf, ft) ** 2 * np.exp(-delta) * acc


def psi2_shared(mu, svec, z, ell, sf, ft=np.float64):
    """Psi2 when every row has the variance vector ``svec``: sf^2 prod_e (1 + 2 s_e / l_e^2)^-1/2 C o (G^T G)."""
    mu, z, svec = _f(mu, ft), _f(z, ft), _f(svec, ft)
    l2 = ells(ell, mu.shape[1], ft) ** 2
    den = l2 + 2 * svec
    g = np.exp(-((mu[:, None, :] - z[None, :, :]) ** 2 / den).sum(axis=2) / 2)
    c = np.exp(-((z[:, None, :] - z[None, :, :]) ** 2 * (svec / (2 * l2 * den))).sum(axis=2))
    return _f(sf, ft) ** 2 * np.prod(1 + 2 * svec / l2) ** _f(-0.5, ft) * c * (g.T @ g)


def tiny(u):
    """The smallest normal number of the format with unit roundoff ``u``: below it a result has no relative accuracy."""
    return float(np.finfo(np.float32 if u > 1e-10 else np.float64).tiny)


def psi1_terms(mu, s, z, ell, sf, roundings=None):
    """(Psi1, w) in longdouble: the entry may be off by u (w + Psi1) (:func:`bound`).  The kernel forms the exponent as
    c0 - sum_e (mu_e - z_e)^2 h_e with c0 and h_e rounded once: c0 carries u |c0|, every step of the sum three roundings
    (the difference, its square, the multiply-add) and h_e's own, all relative to a part of t, so the exponent is off by
    at most (3 d + 2) u t (``roundings`` = 3 d + 2); then the exponential, the product with sf and the stored value:
    2 d + 12 covers them with the margin the Psi2 bound has."""
    ld = np.longdouble
    p, t = psi1_parts(mu, s, z, ell, sf, ld)
    d = np.shape(mu)[1]
    return p, p * ((3 * d + 2 if roundings is None else roundings) * t + 2 * d + 12)


def psi2_terms(mu, s, z, ell, sf, roundings=None):
    """(Psi2, w) in longdouble, w = sum_i term_ijk [n + (3 d + 2)(t_ijk + delta_jk) + 2 d + 12], all terms positive: the entry
    may be off by u (w + Psi2) (:func:`bound`).  ``roundings``: the roundings per unit of exponent, 3 d + 2 by default."""
    ld = np.longdouble
    n, d = np.shape(mu)
    k = 3 * d + 2 if roundings is None else roundings
    delta = psi2_delta(z, ell, ld)
    acc = np.zeros(delta.shape, dtype=ld)
    werr = np.zeros(delta.shape, dtype=ld)
    for t in psi2_rows(mu, s, z, ell, ld):
        e = np.exp(-t)
        acc += e
        werr += e * (n + k * (t + delta) + 2 * d + 12)
    scale = _f(sf, ld) ** 2 * np.exp(-delta)
    return scale * acc, scale * werr


def bound(p, w, u, terms=1):
    """What a stored entry of value ``p`` may be off by in the format of unit roundoff ``u``: u w for the roundings on the way,
    u p for the stored value's own, and the format's underflow floor once per term of the sum."""
    return np.asarray(u * w + u * p + (terms + 2) * tiny(u), dtype=np.float64)


def gauss_hermite(mu, s, z, ell, sf, nodes=40):
    """(E k(x_i, z_j), sum_i E k(z_j, x_i) k(x_i, z_k)) by a nodes^d Gauss-Hermite rule, d <= 2, float64."""
    mu, s, z = _f(mu, np.float64), _f(s, np.float64), _f(z, np.float64)
    n, d = mu.shape
    assert d <= 2
    t, w = np.polynomial.hermite.hermgauss(nodes)
    w = w / np.sqrt(np.pi)
    grids = np.meshgrid(*([t] * d), indexing="ij")
    pts = np.stack([g.ravel() for g in grids], axis=1)                  # (nodes^d, d)
    wts = np.prod(np.stack(np.meshgrid(*([w] * d), indexing="ij"), axis=0), axis=0).ravel()
    p1 = np.zeros((n, z.shape[0]))
    p2 = np.zeros((z.shape[0], z.shape[0]))
    for i in range(n):
        x = mu[i] + np.sqrt(2 * s[i]) * pts
        k = kern(x, z, ell, sf)                                          # (nodes^d, m)
        p1[i] = wts @ k
        p2 += (k * wts[:, None]).T @ k
    return p1, p2


# ------------------------------------------------------------------------------------------ linear algebra in ft ----
def chol(a):
    """The lower Cholesky factor, column by column, in a's float type."""
    a = np.array(a, copy=True)
    m = a.shape[0]
    l = np.zeros_like(a)
    for j in range(m):
        v = a[j:, j] - l[j:, :j] @ l[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        l[j:, j] = v / np.sqrt(v[0])
    return l


def solve_lower(l, b):
    """L^-1 b by forward substitution."""
    b = np.array(b, copy=True)
    x = np.zeros_like(b)
    for i in range(l.shape[0]):
        x[i] = (b[i] - l[i, :i] @ x[:i]) / l[i, i]
    return x


class Model(object):
    """The collapsed bound and the prediction of the sparse GP on uncertain inputs in float type ``ft``: ``s`` an (n, d)
    array of input variances (a (d,) vector or a scalar is broadcast)."""

    def __init__(self, mu, s, z, y, ell, sf, noise, eps=1e-6, ft=np.float64):
        self.ft = ft
        mu, z, y = _f(mu, ft), _f(z, ft), _f(y, ft)
        n, d = mu.shape
        s = np.broadcast_to(_f(s, ft), (n, d))
        m, q = z.shape[0], y.shape[1]
        sf, noise = _f(sf, ft), _f(noise, ft)
        self.mu, self.s, self.z, self.ell, self.sf, self.noise = mu, s, z, ell, sf, noise
        kuu = kern(z, z, ell, sf, ft) + _f(eps, ft) * sf * np.eye(m, dtype=ft)
        self.lu = chol(kuu)
        p1, p2 = psi1(mu, s, z, ell, sf, ft), psi2(mu, s, z, ell, sf, ft)
        x1 = solve_lower(self.lu, p2)
        t = solve_lower(self.lu, x1.T)
        t = (t + t.T) / 2
        self.lb = chol(np.eye(m, dtype=ft) + t / noise)
        c = solve_lower(self.lu, p1.T @ y) / noise
        self.gamma = solve_lower(self.lb, c)
        two_pi = 2 * _f(np.pi, ft) if ft is np.float64 else 8 * np.arctan(_f(1, ft))
        self.bound = (-_f(n * q, ft) / 2 * np.log(two_pi * noise) - q * np.log(np.diagonal(self.lb)).sum() - (y ** 2).sum() / (2 * noise)
                      + (self.gamma ** 2).sum() / 2 - q * (n * sf - np.trace(t)) / (2 * noise))
        pos = s > 0
        safe = np.where(pos, s, _f(1, ft))
        self.kl = (np.where(pos, safe + mu ** 2 - 1 - np.log(safe), _f(0, ft))).sum() / 2
        self.elbo = self.bound - self.kl

    def _tail(self, kstar, want_var, include_noise):
        a = solve_lower(self.lu, kstar.T).T
        w = solve_lower(self.lb, a.T).T
        mean = w @ self.gamma
        if not want_var:
            return mean, None
        var = self.sf - (a ** 2).sum(axis=1) + (w ** 2).sum(axis=1) + (self.noise if include_noise else 0)
        return mean, var

    def predict(self, xs, include_noise=False):
        return self._tail(kern(xs, self.z, self.ell, self.sf, self.ft), True, include_noise)

    def predict_uncertain(self, xs, xs_var):
        xs = _f(xs, self.ft)
        sv = np.broadcast_to(_f(xs_var, self.ft), xs.shape)
        return self._tail(psi1(xs, sv, self.z, self.ell, self.sf, self.ft), False, False)[0]


def both(*args, **kw):
    """(float64 model, longdouble model) of the same problem."""
    return Model(*args, ft=np.float64, **kw), Model(*args, ft=np.longdouble, **kw)


def allowance(v64, vld, factor=10.0, floor=1e-10):
    """What a device value may be off the longdouble value ``vld``: ``factor`` x |float64 - longdouble| of that quantity
    (the factor covers the device's other summation order), never less than ``floor`` relative."""
    v64, vld = np.asarray(v64, dtype=np.longdouble), np.asarray(vld, dtype=np.longdouble)
    return np.asarray(np.maximum(factor * np.abs(v64 - vld), floor * np.abs(vld)), dtype=np.float64)


def slices(n, m, tile=64, target=2048, min_slice=64, align=16):
    """(S, slice length) by the rule of include/cimrgp_psi.h."""
    t = -(-m // tile)
    tiles = t * (t + 1) // 2
    s0 = max(1, min(target // tiles, -(-n // min_slice)))
    length = -(-(-(-n // s0)) // align) * align
    return -(-n // length), length


def scratch_bytes(esz, n, m, d):
    """cimrgp_psi2_scratch_bytes: the counts, the rows' constants and the partial tiles, each part a multiple of 16 bytes."""
    t = -(-m // 64)
    r16 = lambda b: -(-b // 16) * 16
    return r16(-(-n // 256) * 8) + r16(n * (2 * d + 1) * esz) + slices(n, m)[0] * (t * (t + 1) // 2) * 4096 * esz


def problem(n, m, d, seed, q=2, far=True, ell0=1.0):
    """(mu, s, z, y): unit-scale inputs; s mixed over four decades with every fifth row exactly 0 and one row at 10^6;
    with ``far`` (m >= 2) two inducing inputs 40 length-scales ``ell0`` apart in the first dimension (their term underflows)."""
    rng = np.random.RandomState(seed)
    mu = rng.randn(n, d)
    s = 10.0 ** rng.uniform(-3, 1, size=(n, d))
    s[::5] = 0.0
    s[n // 2] = 1e6
    z = rng.randn(m, d)
    if far and m >= 2:
        z[0, 0], z[m - 1, 0] = -20.0 * ell0, 20.0 * ell0
    y = np.sin(mu @ rng.randn(d, q)) + 0.1 * rng.randn(n, q)
    return mu, s, z, y
