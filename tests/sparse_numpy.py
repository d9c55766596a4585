"""NumPy restatement of the inducing-point sparse GP (include/cimrgp_sparse.h, DESIGN.md "Sparse (inducing-point) GP
regression"), shared by tests/test_sparse_host.py and the GPU tests.  Two independent forms: the Woodbury chain the
device runs, and the dense definition K~ = Q_ff + Lambda solved as an n x n system.  Covariance ids are those of
include/cimrgp.h (CIMRGP_COV_*); mode 0 = FITC, 1 = VFE."""
import numpy as np
import scipy.linalg as sla

from grad_numpy import kcov, rel  # noqa: F401  (rel is re-exported)


def _chol_uu(z, cov, ell, sf2, eps):
    return np.linalg.cholesky(kcov(z, z, cov, ell, sf2) + eps * sf2 * np.eye(z.shape[0]))


def _a_of(x, z, lu, cov, ell, sf2):
    """A = K(x, z) L_u^-T."""
    return sla.solve_triangular(lu, kcov(x, z, cov, ell, sf2).T, lower=True).T


def woodbury(x, z, r, cov, ell, sf2, noise, eps, mode, xs=None, include_noise=False):
    """(lml, mean*, var*) by the chain of the issue; mean* / var* are None without xs."""
    n, q = r.shape
    m = z.shape[0]
    lu = _chol_uu(z, cov, ell, sf2, eps)
    a = _a_of(x, z, lu, cov, ell, sf2)
    qd = (a * a).sum(axis=1)
    lam = (sf2 - qd + noise) if mode == 0 else np.full(n, float(noise))
    if not (lam > 0).all():
        raise np.linalg.LinAlgError("lambda not positive")
    aw = a / lam[:, None]
    lb = np.linalg.cholesky(np.eye(m) + a.T @ aw)
    gamma = sla.solve_triangular(lb, aw.T @ r, lower=True)
    lml = (-0.5 * n * q * np.log(2 * np.pi) - 0.5 * q * np.log(lam).sum() - q * np.log(np.diag(lb)).sum()
           - 0.5 * (r * r / lam[:, None]).sum() + 0.5 * (gamma * gamma).sum())
    if mode == 1:
        lml -= 0.5 * q * (sf2 - qd).sum() / noise
    if xs is None:
        return lml, None, None
    as_ = _a_of(xs, z, lu, cov, ell, sf2)
    ws = sla.solve_triangular(lb, as_.T, lower=True).T
    var = sf2 - (as_ * as_).sum(axis=1) + (ws * ws).sum(axis=1) + (noise if include_noise else 0.0)
    return lml, ws @ gamma, var


def dense(x, z, r, cov, ell, sf2, noise, eps, mode, xs=None, include_noise=False):
    """The same from the definition: K~ = Q_ff + Lambda (n x n), Q = K_.u (K_uu + eps sf I)^-1 K_u.;
    LML = log N(r | 0, K~) (- the trace term for VFE); mean* = Q_*f K~^-1 r, var* = sf - Q_** + Q_** - Q_*f K~^-1 Q_f*."""
    n, q = r.shape
    kuu = kcov(z, z, cov, ell, sf2) + eps * sf2 * np.eye(z.shape[0])
    kfu = kcov(x, z, cov, ell, sf2)
    qff = kfu @ np.linalg.solve(kuu, kfu.T)
    qd = np.diag(qff)
    lam = (sf2 - qd + noise) if mode == 0 else np.full(n, float(noise))
    kt = qff + np.diag(lam)
    lt = np.linalg.cholesky(kt)
    alpha = sla.cho_solve((lt, True), r)
    lml = -0.5 * n * q * np.log(2 * np.pi) - q * np.log(np.diag(lt)).sum() - 0.5 * (r * alpha).sum()
    if mode == 1:
        lml -= 0.5 * q * (sf2 - qd).sum() / noise
    if xs is None:
        return lml, None, None
    ksu = kcov(xs, z, cov, ell, sf2)
    qsf = ksu @ np.linalg.solve(kuu, kfu.T)
    v = sla.solve_triangular(lt, qsf.T, lower=True)
    var = sf2 - (v * v).sum(axis=0) + (noise if include_noise else 0.0)
    return lml, qsf @ alpha, var


def exact(x, r, cov, ell, sf2, noise, xs):
    """The exact GP: (lml, mean*, latent var*)."""
    n, q = r.shape
    lower = np.linalg.cholesky(kcov(x, x, cov, ell, sf2) + noise * np.eye(n))
    alpha = sla.cho_solve((lower, True), r)
    lml = -0.5 * n * q * np.log(2 * np.pi) - q * np.log(np.diag(lower)).sum() - 0.5 * (r * alpha).sum()
    ks = kcov(xs, x, cov, ell, sf2)
    v = sla.solve_triangular(lower, ks.T, lower=True)
    return lml, ks @ alpha, sf2 - (v * v).sum(axis=0)


def wsyrk(a, w, r=None, diag_add=0.0):
    """(C, g, bound_C, bound_g): C = diag_add I + A^T diag(w) A, g = A^T diag(w) r and the sums of magnitudes
    sum_k |w_k A_ki A_kj| that the componentwise error bound (n + 2) u sum |.| scales."""
    aw = a * w[:, None]
    c = a.T @ aw + diag_add * np.eye(a.shape[1])
    bc = np.abs(a).T @ np.abs(aw)
    if r is None:
        return c, None, bc, None
    return c, aw.T @ r, bc, np.abs(aw).T @ np.abs(r)


def slices(n, m):
    """(S, slice length) of cimrgp_wsyrk_tn by its rule: tiles x S <= 1024, a slice of at least 256 rows, slice starts
    on multiples of 32."""
    t = (m + 127) // 128
    tiles = t * (t + 1) // 2
    s = max(1, min(1024 // tiles, (n + 255) // 256))
    length = ((n + s - 1) // s + 31) // 32 * 32
    return (n + length - 1) // length, length


def scratch_bytes(esz, n, m, q):
    """cimrgp_wsyrk_tn_scratch_bytes by its formula."""
    t = (m + 127) // 128
    s = slices(n, m)[0]
    return esz * s * (t * (t + 1) // 2 * 128 * 128 + (t * 128 * 8 if q > 0 else 0))


def problem(n, m, d, seed, q=2):
    """Inputs of the acceptance sets: x uniform on [-2, 2]^d, a smooth target plus noise, Z a random subset."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, size=(n, d))
    f = np.stack([np.sin(2 * x).sum(axis=1), np.cos(x).prod(axis=1)], axis=1)[:, :q]
    r = f + 0.1 * rng.normal(size=(n, q))
    z = x[rng.permutation(n)[:m]]
    xs = rng.uniform(-2.2, 2.2, size=(257, d))
    return x, z, r, xs
