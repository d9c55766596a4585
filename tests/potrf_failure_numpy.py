"""A failing Cholesky pivot that is exact by construction, and the cases the failure tests share.

The base matrix K is the RBF Gram of sorted one-dimensional uniform points on [-2, 2] with ell = 0.05, sf2 = 1 and
noise = 0.1 (the parameters of test_potrf_f32_lookahead_backward_error: safe in FP32).  Overwriting K[j-1, j-1] with a
value <= 0 leaves every leading minor of order < j untouched; every earlier Schur pivot is at least
lambda_min(K) >= noise = 0.1, far above the rounding of either precision, and pivot j is at most the injected value.
So LAPACK's ``info`` -- and the library's -- is j exactly, in FP64 and in FP32, with no +-1 from rounding (a duplicated
point with zero noise moves the failing pivot by one).  test_potrf_failure_host.py checks that claim against dpotrf and
spotrf for every case below; test_gpu_potrf_failure.py runs the same cases through the HIP factorisation.

Case lists name the schedule path each case reaches (cimrgp_amd/csrc/potrf.hip; the thresholds are Knobs in common.hpp
and SINGLE_QUEUE_MAX).
"""
import numpy as np

import oracle

ELL, SF2, NOISE = 0.05, 1.0, 0.1
SB, NB = 64, 256                       # columns per diagonal block / per panel (CIMRGP_NB)
NAN = float("nan")


def points(n, seed=None):
    """Sorted uniform points on [-2, 2], (n x 1); the seed defaults to n."""
    rng = np.random.default_rng(n if seed is None else seed)
    return np.sort(rng.uniform(-2.0, 2.0, size=(n, 1)), axis=0)


def base_gram(x):
    return oracle.rbf_gram(x, None, ELL, SF2, NOISE)


def inject(k, injections):
    """A copy of k with k[j-1, j-1] = value for every (j, value)."""
    out = np.array(k, copy=True)
    for j, value in injections:
        out[j - 1, j - 1] = value
    return out


def expected_info(injections):
    """LAPACK's info: the order of the first leading minor that is not positive definite."""
    return min(j for j, _ in injections)


def block_start(j):
    """c0: first column of the 64-column block that holds column j-1.  Columns of L left of it are final."""
    return SB * ((j - 1) // SB)


def panel_start(j):
    """k0: first column of the 256-column panel that holds column j-1.  Carried rows' columns left of it are final."""
    return NB * ((j - 1) // NB)


def carried_rows(n, m):
    return np.random.default_rng(1000 * n + m).normal(size=(m, n))


# ---- one queue (n <= 5120): fused_sweep, nine-wave k_diag64 (first block of a panel) and k_link (blocks 1..3) --------
# (n, m, injections); n = 700 is three panels, the last 188 wide (blocks of 64, 64 and 60)
ONE_QUEUE = [(700, 0, ((j, -1.0),)) for j in (
    1,        # k_diag64, panel 0, first lane
    2,
    64,       # last lane of a block
    65,       # first block handled by k_link
    193,      # k_link, last block of panel 0
    256,      # last column of a panel
    257,      # k_diag64 with a left-looking prologue (the previous panel's last sub-block)
    448,      # k_link in panel 1
    641,      # first column of the ragged last block, w = 60 (k_link: block 2 of panel 2)
    700,      # last column, inside the lane < w guard
)] + [
    (641, 0, ((641, -1.0),)),                  # last block w = 1 beside 63 padding lanes
    (700, 0, ((1, 0.0),)),                     # an exactly zero pivot
    (700, 0, ((300, NAN),)),                   # not a number: the first pivot that is not positive (!(d > 0))
    (700, 0, ((100, -1.0), (500, -1.0))),      # two bad pivots: the first one is reported
] + [(700, 70, ((j, -1.0),)) for j in (65, 257, 700)]          # carried rows solved along by the chain's launches

# ---- look-ahead (n = 6144 > 5120): LookAheadRun.  24 panels.
# Without rows the one-queue tail starts once n - k1 <= tail_below = 4864: the steps at k0 = 0 .. 768 factor panels
# 1 .. 4 (columns 256 .. 1279) with the four-wave kernels, tail(1024) factors the columns from 1280 on (nine-wave).
# With rows the tail starts once n - k1 <= rows_beside_tail_below = 2560: look-ahead through column 3583, tail from 3584.
LOOKAHEAD_N = 6144
LOOKAHEAD_M = (0, 130)
LOOKAHEAD_J = (
    100,      # panel 0: nine-wave, started ahead of everything else (LookAheadRun.start), k_link
    300,      # panel 1: four-wave k_diag64q (first block of a look-ahead panel); gated step in FP64 without rows
    700,      # panel 2: four-wave k_linkq
    1300,     # first tail panel without rows (columns 1280 .. 1535); still look-ahead with rows
    3000,     # tail without rows; look-ahead beside the running rows queues with rows
    4000,     # tail either way (from column 3584 with rows)
    6144,     # last column
)

# ---- paired far updates: n = 10240 > far_pair_above = 8192: the steps at k0 = 0 .. 1280 update the far part once per
# two panels (K = 512); j = 5000 lies in panel 4864, factored by the look-ahead step at k0 = 4608 (tail from 5376)
PAIRED = (10240, 5000)

# ---- batched: (n, batch, {block: j}).  Blocks not named are clean.
BATCHED = [
    # 3 x 320 / 32 = 30 chain workgroups <= fused_max_chain_wgs: fused_sweep with riders, four-wave kernels
    (320, 3, {0: 65, 2: 320}),
    # 25 x 32 = 800 > 768 and 25 >= batch_halves_min: two halves (blocks 0..11, 12..24) on two queues, panel_sweep
    (1024, 25, {11: 257, 12: 1, 24: 1024}),
    # 7 x 112 = 784 > 768, 7 < batch_halves_min: panel_sweep<T, true> on one queue
    (3584, 7, {6: 2000}),
]

# ---- staged pipeline: the failure comes through the inputs (the call builds its own Gram matrix).  Evenly spaced
# points with x[j-1] = x[j-2], ell about the spacing, no noise: dpotrf gives exactly j on the CPU, the matrix without the
# duplicate is well conditioned (smallest pivot 0.57).
STAGED_N, STAGED_J, STAGED_ELL = 5632, 3000, 7e-4


def staged_bad_points():
    x = np.linspace(-2.0, 2.0, STAGED_N).reshape(-1, 1)
    x[STAGED_J - 1] = x[STAGED_J - 2]
    return x


def single_cases():
    """Every single-matrix case as (n, m, injections)."""
    out = list(ONE_QUEUE)
    for m in LOOKAHEAD_M:
        out += [(LOOKAHEAD_N, m, ((j, -1.0),)) for j in LOOKAHEAD_J]
    out.append((PAIRED[0], 0, ((PAIRED[1], -1.0),)))
    return out


def batch_seed(n, block):
    """Seed of block `block`'s points in a batched case."""
    return 100 * n + block


def host_cases():
    """The distinct (n, seed, injections) of the GPU file that LAPACK confirms on the CPU: n <= 6144 and injected
    values -1.0 or 0.0 (`seed`: of the points, see points())."""
    seen, out = set(), []
    cases = [(n, n, inj) for n, _, inj in single_cases()]
    cases += [(n, batch_seed(n, blk), ((j, -1.0),)) for n, _, bad in BATCHED for blk, j in sorted(bad.items())]
    for case in cases:
        n, _, inj = case
        if n > 6144 or any(v not in (-1.0, 0.0) for _, v in inj) or case in seen:
            continue
        seen.add(case)
        out.append(case)
    return out
