"""Dense, well-conditioned SPD matrices on which every 256-tile of the Cholesky factor counts, the acceptance rules
for factorisations and triangular solves on them, and the cases test_gpu_dense_spd.py runs.

Why: every other matrix the suite factors is an RBF Gram of sorted one-dimensional points with a short length-scale.
Such a matrix and its factor are numerically banded (max |L| is 1e-9 beyond 512 rows of the diagonal and 1e-40 beyond
1024 at n = 5632, ell = 0.05), so a far trailing-update tile that is skipped, applied twice, reads the wrong operand
block or loses a race changes nothing a tolerance can see.  Here no tile is small:

  low-rank form   K = I + G G^T / r, G (n x r) standard normal, r = 32.  lambda_min = 1 exactly (n > r) and
                  lambda_max = 1 + s_max(G)^2 / r <= 1 + (1 + sqrt(n / r))^2 (s_max(G) <= sqrt(n) + sqrt(r) but for a
                  probability below exp(-t^2 / 2) at sqrt(n) + sqrt(r) + t; lowrank_spd rejects a draw that misses it).
  kernel form     the RBF Gram of sorted uniform points on [-2, 2] at ell = 2.0, sf2 = 1.0, noise = 1.0, for the entries
                  that build their own Gram matrix.  lambda_min >= noise and lambda_max <= noise + n sf2 (the trace).
                  (ell = 0.5 does not serve: the far tiles of L fall to 1e-12.)

tile_weight() is the condition every matrix a test uses must meet (>= MIN_TILE_WEIGHT): the smallest, over the lower
256-tiles of L, of max |L_tile| / max |L|.

Acceptance rules, shared by the host tests (on blocked_cholesky / rows_solve below, clean and mutated) and the GPU tests
(on the library):

  FP64 factor   rho = max_{i >= j} |L L^T - K|_ij / (gamma_{n+1} sqrt(kappa) (|L| |L|^T)_ij) <= 1, gamma_k = k u / (1 - k u),
                u = 2^-53, kappa the bound on cond(K) above.  The componentwise bound |K - L L^T| <= gamma_{n+1} |L| |L|^T
                of the Cholesky factorisation holds for every order of summation (matrix-core accumulation included); the
                panels are solved with explicitly inverted diagonal blocks, which costs a factor cond(L) = sqrt(cond(K)).
  FP64 solves   the same for the residual of the triangular system: |W L^T - B|_ij against (|W| |L^T|)_ij for W = B L^-T,
                |X L - B|_ij against (|X| |L|)_ij for X = B L^-1; a forward solve L z = r is the first form on z^T, a
                backward solve L^T a = z the second on a^T.
  FP32          the derived bound is too wide to see a single dropped term (gamma ~ 5e-4 at n = 8192), so the rule is
                measured: the max-norm relative forward error against the FP64 oracle of the same FP32-rounded inputs
                must be at most FP32_MARGIN = 8 times the error the reference FP32 routine (LAPACK through SciPy, or
                torch's float32 linalg) makes on those inputs.  The margin covers what legitimately differs from LAPACK:
                the blocked order, the inverted blocks, the matrix-core accumulation.

Everything takes NumPy arrays (LAPACK through SciPy, on the host) or torch tensors (torch.linalg, on the tensor's
device); torch is imported where it is used, and nothing here touches the library under test.
"""
import json
import os

import numpy as np
import scipy.linalg as sla

NB = 256                                # tile of the reports and of tile_weight: the library's panel width (CIMRGP_NB)
RANK = 32
U64 = 2.0 ** -53
MIN_TILE_WEIGHT = 1e-3
FP32_MARGIN = 8.0
KERNEL_ELL, KERNEL_SF2, KERNEL_NOISE = 2.0, 1.0, 1.0
HOST_ORACLE_MAX = 6144                  # the oracle's factor is LAPACK on the host up to here, torch.linalg on the device above
MUTATIONS = ("skip", "double", "drop_one_k", "neighbour_operand")


# ---- matrices --------------------------------------------------------------------------------------------------------

def lowrank_draws(n, seed, r=RANK):
    """(G, number of rejected draws): G (n x r) standard normal, the first draw of default_rng(seed) whose K meets the cond
    bound.  The bound sits about one percent above the typical cond, so now and then a draw misses it."""
    rng = np.random.default_rng(seed)
    rejected = 0
    while True:
        g = rng.standard_normal((n, r))
        if lowrank_cond(g) <= lowrank_cond_bound(n, r):
            return g, rejected
        rejected += 1


def lowrank_spd(n, seed, r=RANK):
    """G (n x r), standard normal: K = I + G G^T / r meets the cond bound (lowrank_draws).  For the cases below the first
    draw is taken but for the four of REDRAWN; test_dense_spd_host.py pins that, so that a change of the bound cannot
    quietly change the matrices."""
    return lowrank_draws(n, seed, r)[0]


def lowrank_matrix(g):
    """K = I + G G^T / r on the host (the GPU tests form it on the device from the uploaded G)."""
    n, r = g.shape
    return np.eye(n) + (g @ g.T) / r


def lowrank_cond_bound(n, r=RANK):
    return 1.0 + (1.0 + np.sqrt(n / r)) ** 2


def lowrank_cond(g):
    """cond(I + G G^T / r), exactly, from G's singular values (lambda_min = 1 for n > r)."""
    n, r = g.shape
    s = np.linalg.svd(g, compute_uv=False)
    lam_min = 1.0 if n > r else 1.0 + s[-1] ** 2 / r
    return (1.0 + s[0] ** 2 / r) / lam_min


def kernel_dense_points(n, seed):
    """Sorted uniform points on [-2, 2], (n x 1), for the kernel form (KERNEL_ELL, KERNEL_SF2, KERNEL_NOISE)."""
    return np.sort(np.random.default_rng(seed).uniform(-2.0, 2.0, size=(n, 1)), axis=0)


def kernel_cond_bound(n):
    return 1.0 + n * KERNEL_SF2 / KERNEL_NOISE


# ---- array plumbing --------------------------------------------------------------------------------------------------

def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def _t64(a):
    """``a`` as a float64 torch tensor (a NumPy array becomes a host tensor)."""
    import torch
    if _is_tensor(a):
        return a.to(torch.float64)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def sym_from_lower(k):
    """The symmetric matrix whose lower triangle is ``k``'s (what a routine that reads the lower triangle factors)."""
    if _is_tensor(k):
        import torch
        low = torch.tril(k)
        return low + torch.tril(k, -1).t()
    low = np.tril(k)
    return low + np.tril(k, -1).T


def _tile_max(a, nb):
    """(row tiles x column tiles) largest entry of each nb x nb tile of the non-negative 2-D tensor ``a``; NaN stays NaN."""
    import torch
    r, c = a.shape
    tr, tc = -(-r // nb), -(-c // nb)
    pad = torch.zeros((tr * nb, tc * nb), dtype=a.dtype, device=a.device)
    pad[:r, :c] = a
    return pad.view(tr, nb, tc, nb).amax(dim=(1, 3))


def tile_weight(lower, nb=NB):
    """The smallest, over the lower nb-tiles of L, of max |L_tile| / max |L|."""
    import torch
    la = torch.tril(_t64(lower)).abs()
    tiles = _tile_max(la, nb)
    mask = torch.tril(torch.ones_like(tiles, dtype=torch.bool))
    return float(tiles[mask].min() / la.max())


# ---- the oracle and the FP32 reference ------------------------------------------------------------------------------------

def factor(k, dtype=np.float64):
    """Lower Cholesky factor of the symmetric ``k`` in ``dtype`` (np.float64: the oracle, np.float32: the reference):
    LAPACK's potrf for a NumPy array, torch.linalg.cholesky on the tensor's device for a tensor.  Raises LinAlgError when
    ``k`` is not positive definite."""
    if _is_tensor(k):
        import torch
        tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        low, info = torch.linalg.cholesky_ex(k.to(tdt))
        if int(info.item()) != 0:
            raise np.linalg.LinAlgError("not positive definite (leading minor of order %d)" % int(info.item()))
        return low
    potrf = sla.lapack.dpotrf if np.dtype(dtype) == np.float64 else sla.lapack.spotrf
    low, info = potrf(np.asarray(k, dtype=dtype), lower=1)
    if info != 0:
        raise np.linalg.LinAlgError("not positive definite (leading minor of order %d)" % info)
    return np.tril(low)


def solve_rows(lower, b, dtype=np.float64, lt=False):
    """W = B L^-T (``lt``: X = B L^-1) in ``dtype``: LAPACK's trsm through SciPy for NumPy arrays, torch.linalg for tensors."""
    if _is_tensor(lower):
        import torch
        tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        low, rhs = lower.to(tdt), b.to(tdt)
        if lt:
            return torch.linalg.solve_triangular(low, rhs, upper=False, left=False)
        return torch.linalg.solve_triangular(low.t(), rhs, upper=True, left=False)
    low, rhs = np.asarray(lower, dtype=dtype), np.asarray(b, dtype=dtype)
    return sla.solve_triangular(low, rhs.T, lower=True, trans="T" if lt else "N", check_finite=False).T


def kinv_diag(lower, dtype=np.float64):
    """diag(K^-1) = squared row norms of L^-T, every step in ``dtype``."""
    n = lower.shape[0]
    if _is_tensor(lower):
        import torch
        eye = torch.eye(n, dtype=lower.dtype, device=lower.device)
    else:
        eye = np.eye(n)
    u = solve_rows(lower, eye, dtype)                 # I L^-T
    return (u * u).sum(1)


def kinv_diag_bound(n, kappa):
    """FP64 bound on max |d - diag(K^-1)| / max diag(K^-1) for d computed from a factor that passes factor_rho <= 1 by
    rows that pass rows_rho <= 1: a row u of L^-T with backward error gamma sqrt(kappa) has forward error
    gamma sqrt(kappa) cond(L) = gamma kappa, so |u|^2 moves by 2 gamma kappa; the factor's own backward error
    gamma sqrt(kappa) moves K^-1 by cond(K) times that.  A worst-case bound: clean results sit five orders inside it
    (1e-14 against 2e-9 at n = 5632), and one mutated update tile lands at 3e-3 or more, six orders outside
    (test_kinv_diag_bound_sees_every_rows_mutant), so it separates the two with room on both sides."""
    return gamma(n + 1) * (2.0 * kappa + kappa ** 1.5)


# ---- acceptance: FP64 -------------------------------------------------------------------------------------------------

def gamma(k, u=U64):
    return k * u / (1.0 - k * u)


def _worst(num, den, scale, nb):
    """rho = max num / (scale den) and the nb-tile that holds it; 0 / 0 counts as 0, x / 0 and NaN as infinite."""
    import torch
    ratio = num / (scale * den)
    ratio = torch.where((den == 0) & (num == 0), torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    tiles = _tile_max(ratio, nb)
    flat = int(torch.argmax(tiles))
    return float(tiles.max()), (flat // tiles.shape[1], flat % tiles.shape[1])


def factor_rho(lower, k, kappa, nb=NB):
    """(rho, (row tile, column tile)) of the FP64 factor rule for K = L L^T; ``k`` symmetric, FP64."""
    import torch
    low = torch.tril(_t64(lower))
    kk = _t64(k).to(low.device)
    n = low.shape[0]
    num = torch.tril((low @ low.t() - kk).abs())
    la = low.abs()
    den = la @ la.t()
    return _worst(num, den, gamma(n + 1) * np.sqrt(kappa), nb)


def rows_rho(w, lower, b, kappa, lt=False, nb=NB):
    """(rho, (row tile, column tile)) of the FP64 rule for W L^T = B (``lt``: W L = B); w and b (m x n)."""
    import torch
    low = torch.tril(_t64(lower))
    ww, bb = _t64(w).to(low.device), _t64(b).to(low.device)
    n = low.shape[0]
    a = low if lt else low.t()
    num = (ww @ a - bb).abs()
    den = ww.abs() @ a.abs()
    return _worst(num, den, gamma(n + 1) * np.sqrt(kappa), nb)


def report(what, rho, tile):
    return "%s: rho = %.3e, worst tile (row tile %d, column tile %d)" % (what, rho, tile[0], tile[1])


# ---- acceptance: FP32 -------------------------------------------------------------------------------------------------

def forward_error(got, want):
    """max |got - want| / max |want|; infinite when ``got`` is not finite."""
    import torch
    w = _t64(want)
    g = _t64(got).to(w.device)
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return float((g - w).abs().max() / w.abs().max())


def fp32_ratio(device_error, reference_error):
    """Device error over reference error: the FP32 rule passes at FP32_MARGIN or below."""
    return device_error / reference_error


# ---- the plain blocked algorithms, with one mutated update --------------------------------------------------------------

def _mutated_product(kind, a, b, a_neighbour):
    """What a mutated update subtracts instead of a b^T."""
    if kind == "skip":
        return None
    if kind == "double":
        return 2.0 * (a @ b.T)
    if kind == "drop_one_k":
        keep = np.arange(a.shape[1]) != a.shape[1] // 2
        return a[:, keep] @ b[:, keep].T
    if kind == "neighbour_operand":
        if a_neighbour is None or a_neighbour.shape != a.shape:
            raise ValueError("no neighbour block of the same shape")
        return a_neighbour @ b.T
    raise ValueError("unknown mutation %r" % (kind,))


def _neighbour(t, p, ntiles):
    """The tile index a wrong operand is taken from: the one before ``t`` if that lies below panel ``p``, else the next."""
    if t - 1 > p:
        return t - 1
    return t + 1 if t + 1 < ntiles else None


def blocked_cholesky(k, nb, mutate=None):
    """Right-looking blocked Cholesky in ``k``'s dtype: for every panel p the diagonal block, the panel solve, then the
    update A_IJ -= L_Ip L_Jp^T of every tile I >= J > p.  ``mutate`` = (kind, p, I, J) changes that one update: ``skip``,
    ``double``, ``drop_one_k`` (the panel's middle column left out) or ``neighbour_operand`` (L_I'p for L_Ip, I' next to I).
    Raises LinAlgError when a diagonal block stops being positive definite."""
    a = np.array(k, copy=True)
    n = a.shape[0]
    nt = -(-n // nb)
    sl = [slice(t * nb, min(n, (t + 1) * nb)) for t in range(nt)]
    for p in range(nt):
        a[sl[p], sl[p]] = factor(sym_from_lower(a[sl[p], sl[p]]), a.dtype)
        if p + 1 == nt:
            break
        below = slice(sl[p].stop, n)
        a[below, sl[p]] = solve_rows(a[sl[p], sl[p]], a[below, sl[p]], a.dtype)
        for i in range(p + 1, nt):
            for j in range(p + 1, i + 1):
                li, lj = a[sl[i], sl[p]], a[sl[j], sl[p]]
                if mutate is not None and tuple(mutate[1:]) == (p, i, j):
                    ni = _neighbour(i, p, nt)
                    prod = _mutated_product(mutate[0], li, lj, None if ni is None else a[sl[ni], sl[p]])
                else:
                    prod = li @ lj.T
                if prod is not None:
                    a[sl[i], sl[j]] -= prod
    return np.tril(a)


def rows_solve(lower, b, nb, mutate=None):
    """Right-looking W = B L^-T in ``b``'s dtype: for every panel p the solve W_p = B_p L_pp^-T, then the update
    B_J -= W_p L_Jp^T of every column tile J > p.  ``mutate`` = (kind, p, J) changes that one update as in
    blocked_cholesky (``neighbour_operand``: L_J'p for L_Jp)."""
    w = np.array(b, copy=True)
    low = np.asarray(lower, dtype=w.dtype)
    n = low.shape[0]
    nt = -(-n // nb)
    sl = [slice(t * nb, min(n, (t + 1) * nb)) for t in range(nt)]
    for p in range(nt):
        w[:, sl[p]] = solve_rows(low[sl[p], sl[p]], w[:, sl[p]], w.dtype)
        for j in range(p + 1, nt):
            lj = low[sl[j], sl[p]]
            if mutate is not None and tuple(mutate[1:]) == (p, j):
                nj = _neighbour(j, p, nt)
                prod = _mutated_product(mutate[0], lj, w[:, sl[p]], None if nj is None else low[sl[nj], sl[p]])
                prod = None if prod is None else prod.T
            else:
                prod = w[:, sl[p]] @ lj.T
            if prod is not None:
                w[:, sl[j]] -= prod
    return w


def diagonal_by_order_f32(lower, kdiag, nb=NB):
    """The order-of-accumulation experiment behind the FP32 finding of test_gpu_dense_spd.py, on the host: the diagonal of
    the factor, l_jj = sqrt(K_jj - sum_{k < j} L_jk^2), with every operation in float32 and the exact off-diagonal entries of
    ``lower`` (FP64) rounded to float32 as terms.  Returns (term_by_term, per_block): the sum subtracted from K_jj one
    product at a time, as update kernels do whose accumulators start as the C tile (n roundings at the size of K_jj); and
    each block of ``nb`` columns summed from zero and subtracted once (n / nb such roundings), as LAPACK's blocked update
    does.  (NumPy rounds the product and the subtraction apart where a matrix core fuses them; the count is what matters.)"""
    low = np.tril(np.asarray(lower, dtype=np.float64), -1).astype(np.float32)
    n = low.shape[0]
    sq = low * low
    seq = np.asarray(kdiag, dtype=np.float32).copy()
    for k in range(n):
        seq -= sq[:, k]
    blk = np.asarray(kdiag, dtype=np.float32).copy()
    for k0 in range(0, n, nb):
        part = np.zeros(n, dtype=np.float32)
        for k in range(k0, min(n, k0 + nb)):
            part += sq[:, k]
        blk -= part
    return np.sqrt(seq), np.sqrt(blk)


# ---- the record ------------------------------------------------------------------------------------------------------

def record(**fields):
    """One JSON line per case, appended to the file CIMRGP_DENSE_SPD_RECORD names (profiles/dense_spd_errors.jsonl is a
    copy of one GPU run's); nothing is written when it is not set."""
    path = os.environ.get("CIMRGP_DENSE_SPD_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(fields, sort_keys=True) + "\n")


# ---- the cases of test_gpu_dense_spd.py ---------------------------------------------------------------------------------
# Each names the schedule path it reaches (cimrgp_amd/csrc/potrf.hip) and the threshold it straddles (Knobs in common.hpp,
# SINGLE_QUEUE_MAX in potrf.hip).  Panels are 256 columns, diagonal blocks 64.  Low-rank form, seed = n, unless noted.

# cimrgp_potrf: (n, path)
POTRF = [
    (700, "one queue: fused_sweep, three panels, ragged last panel (188 = 64 + 64 + 60)"),
    (5120, "one queue: the last size at SINGLE_QUEUE_MAX = 5120, twenty panels, far updates as riders of the chain's launches"),
    (5184, "look-ahead just above SINGLE_QUEUE_MAX: LookAheadRun, panel 0 ahead, tail from n - k1 <= tail_below = 4864 "
           "(tail(256)), 64-column last panel"),
    (5377, "look-ahead, 5377 - 512 = 4865 is one column above tail_below = 4864: one more look-ahead step than 5184, "
           "tail(512); 1-column last panel"),
    (6144, "look-ahead steps at k0 = 0 .. 768 (gated in FP64: persistent head + bulk update), then the one-queue tail from "
           "column 1280 (n - 1280 = tail_below), whose far updates run as FarBulk on the chain queue while "
           ">= tail_far_min_rows = 2048 rows remain"),
    (8192, "the flagship: look-ahead steps at k0 = 0 .. 2816 with the persistent bulk update, then the fused tail(3072) "
           "with FAR(prev) on the second queue; n - k3 = 7424 <= far_pair_above = 8192 at k0 = 0: no paired far update"),
    (9216, "smallest n with one paired far group: n - k3 = 8448 > far_pair_above = 8192 at k0 = 0 only (K = 512 update)"),
    (10240, "paired far updates at k0 = 0 .. 1280 (three groups of two panels, K = 512), then single steps and the tail"),
]

# cimrgp_potrf_rows: (n, m, path); B (m x n) standard normal, seed 1000 n + m
POTRF_ROWS = [
    (700, 70, "one queue: the carried rows solved along in the chain's launches"),
    (6144, 130, "look-ahead with rows on their own queues (rows_pipelined: far update on the second rows queue, persistent "
                "128-row tiles, m just beyond one tile), tail beside the running rows once n - k1 <= "
                "rows_beside_tail_below = 2560 (from column 3584)"),
    (6144, 260, "as above, m just beyond two 128-row tiles of the rows' far update"),
    (6144, 385, "as above, m just beyond three 128-row tiles"),
    (10240, 130, "paired far updates of the matrix and grouped rows (rows_grouped): the rows' far updates take two panels "
                 "at a time (K = 512) while n - r2 > rows_pair_above = 8192"),
]

# solves on a dense factor: n; 5632 > 5120: the backward solves use the paired off-diagonal inverse blocks (bwd_pairs)
SOLVES_N = (700, 2500, 5632)
SOLVE_Q = (1, 3, 8)
SOLVE_M = (15, 129, 1000)

# cimrgp_potrf_rows_batched: (n, batch, path) -- the three batched paths of potrf_failure_numpy.BATCHED; block b's seed is
# batch_seed(n, b)
BATCHED = [
    (320, 3, "3 x 320 / 32 = 30 chain workgroups <= fused_max_chain_wgs = 768: fused_sweep with riders"),
    (1024, 25, "25 x 32 = 800 > fused_max_chain_wgs and 25 >= batch_halves_min = 8: two halves (blocks 0..11, 12..24) on two "
               "queues, panel_sweep"),
    (3584, 7, "7 x 112 = 784 > fused_max_chain_wgs, 7 < batch_halves_min: panel_sweep on one queue"),
]
BATCHED_M = (0, 2)

# entries that build their own Gram matrix (kernel form, FP64): (entry, n, path)
BLOCK_POSTERIOR = [
    (1100, "cimrgp_block_posterior, one queue, ns + q carried rows in the chain's launches"),
    (5377, "cimrgp_block_posterior, look-ahead with carried rows, 1-column last panel"),
]
STAGED = [
    (5632, "cimrgp_block_posterior_staged over two buffer sets, look-ahead with carried rows"),
    (8192, "cimrgp_block_posterior_staged over two buffer sets, the flagship size: persistent bulk update, rows on their queues"),
]
LAYER = (4, 1300, "cimrgp_layer_fit + cimrgp_layer_predict: 4 x 1300 / 32 = 162 chain workgroups, batched fused_sweep with "
                  "riders, q carried rows")


def batch_seed(n, block):
    return 100 * n + block


# (n, seed) -> rejected draws, for the only matrices of the tables above whose first draw misses the cond bound
REDRAWN = {(1024, batch_seed(1024, 1)): 1, (1024, batch_seed(1024, 12)): 1, (3584, batch_seed(3584, 3)): 1, (3584, batch_seed(3584, 4)): 1}


def lowrank_table():
    """(n, seed) of every low-rank matrix of the GPU file."""
    out = [(n, n) for n in sorted({c[0] for c in POTRF} | {c[0] for c in POTRF_ROWS} | set(SOLVES_N))]
    for n, batch, _ in BATCHED:
        out += [(n, batch_seed(n, b)) for b in range(batch)]
    return out


def carried_rows(n, m):
    return np.random.default_rng(1000 * n + m).standard_normal((m, n))


def host_condition_sizes():
    """(form, n, seed) of every matrix of the GPU file up to HOST_ORACLE_MAX: the host test asserts tile weight and
    cond bound on each (the larger ones are asserted in the GPU tests on the oracle's factor)."""
    out = []
    for n in sorted({c[0] for c in POTRF} | {c[0] for c in POTRF_ROWS} | set(SOLVES_N)):
        if n <= HOST_ORACLE_MAX:
            out.append(("lowrank", n, n))
    for n, batch, _ in BATCHED:
        out += [("lowrank", n, batch_seed(n, b)) for b in range(batch)]
    for n in sorted({c[0] for c in BLOCK_POSTERIOR} | {c[0] for c in STAGED} | {LAYER[1]}):
        if n <= HOST_ORACLE_MAX:
            out.append(("kernel", n, n))
    return out
