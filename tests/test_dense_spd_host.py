"""The tests of the dense-SPD tests (tests/dense_spd.py), on the host: the acceptance rules pass the clean blocked
algorithms and fail every mutant of ONE tile's update by ONE panel, in FP64 (rho >= 1e3 against the pass limit 1) and in
FP32 (forward error >= 10 times the pass limit, i.e. 80 times LAPACK's); and every matrix the GPU file uses (up to
n = 6144 here) meets the tile-weight condition and its cond bound.

n = 1536 is six panels of 256.  The figures are printed (outside pytest's capture) so that a run shows the margins."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import dense_spd as ds
import oracle

N, NB = 1536, ds.NB
KAPPA = ds.lowrank_cond_bound(N)

# (panel, row tile, column tile) of the mutated update
FACTOR_TILES = [
    (0, 5, 1),      # the farthest tile, by the first panel
    (2, 5, 5),      # a last-row diagonal tile, by a middle panel
    (2, 4, 3),      # a tile adjacent to the diagonal, by the last panel that touches it
    (0, 1, 1),      # the first diagonal tile behind the first panel
]
# (panel, column tile)
ROWS_TILES = [
    (0, 5),         # the last column tile, by the first panel
    (3, 4),         # the column tile next to the panel
    (3, 5),         # the last column tile, by the last panel but one
]
M_ROWS = 70


@pytest.fixture(scope="module")
def data():
    """K (FP64 and FP32-rounded), their oracle factors, LAPACK's FP32 factor and its error; B and the rows likewise."""
    g = ds.lowrank_spd(N, N)
    k64 = ds.lowrank_matrix(g)
    k32 = k64.astype(np.float32)
    b64 = ds.carried_rows(N, M_ROWS)
    b32 = b64.astype(np.float32)
    l64 = ds.factor(k64)
    l32_oracle = ds.factor(k32.astype(np.float64))                   # FP64 oracle of the FP32-rounded input
    l32_lapack = ds.factor(k32, np.float32)
    w32_oracle = ds.solve_rows(l32_lapack.astype(np.float64), b32.astype(np.float64))
    w32_lapack = ds.solve_rows(l32_lapack, b32, np.float32)
    return dict(g=g, k64=k64, k32=k32, b64=b64, b32=b32, l64=l64, l32_oracle=l32_oracle, l32_lapack=l32_lapack,
                factor_ref_err=ds.forward_error(l32_lapack, l32_oracle),
                w32_oracle=w32_oracle, rows_ref_err=ds.forward_error(w32_lapack, w32_oracle))


def _say(capsys, text):
    with capsys.disabled():
        print("\n  " + text, end="")


def test_the_matrix_meets_its_conditions(data, capsys):
    cond = ds.lowrank_cond(data["g"])
    tw = ds.tile_weight(data["l64"])
    _say(capsys, "n = %d: cond %.1f (bound %.1f), tile weight %.2e, LAPACK FP32 factor error %.2e, rows error %.2e"
         % (N, cond, KAPPA, tw, data["factor_ref_err"], data["rows_ref_err"]))
    assert cond <= KAPPA
    assert tw >= ds.MIN_TILE_WEIGHT


def test_the_old_suites_matrix_fails_the_tile_weight_condition():
    """The RBF Gram of sorted points at ell = 0.05 (every schedule test before this file): numerically banded."""
    x = ds.kernel_dense_points(N, N)
    low = ds.factor(oracle.rbf_gram(x, None, 0.05, 1.0, 0.01))
    assert ds.tile_weight(low) < 1e-30


def test_clean_blocked_cholesky_passes(data, capsys):
    low = ds.blocked_cholesky(data["k64"], NB)
    rho, tile = ds.factor_rho(low, data["k64"], KAPPA)
    low32 = ds.blocked_cholesky(data["k32"], NB)
    assert low32.dtype == np.float32
    err = ds.forward_error(low32, data["l32_oracle"])
    ratio = ds.fp32_ratio(err, data["factor_ref_err"])
    _say(capsys, "clean blocked_cholesky: FP64 %s; FP32 error %.2e = %.2f x LAPACK's" % (ds.report("factor", rho, tile), err, ratio))
    assert rho <= 1.0
    assert ratio <= ds.FP32_MARGIN
    # LAPACK's own factor passes the FP64 rule as well, and the rule sees a symmetric K only through its lower triangle
    rho_lapack, _ = ds.factor_rho(data["l64"], ds.sym_from_lower(np.tril(data["k64"])), KAPPA)
    assert rho_lapack <= 1.0


def test_clean_rows_solve_passes(data, capsys):
    w = ds.rows_solve(data["l64"], data["b64"], NB)
    rho, tile = ds.rows_rho(w, data["l64"], data["b64"], KAPPA)
    w32 = ds.rows_solve(data["l32_lapack"], data["b32"], NB)
    assert w32.dtype == np.float32
    err = ds.forward_error(w32, data["w32_oracle"])
    ratio = ds.fp32_ratio(err, data["rows_ref_err"])
    _say(capsys, "clean rows_solve: FP64 %s; FP32 error %.2e = %.2f x LAPACK's" % (ds.report("rows", rho, tile), err, ratio))
    assert rho <= 1.0
    assert ratio <= ds.FP32_MARGIN
    # the other triangular form, X L = B, on LAPACK's own solve
    x = ds.solve_rows(data["l64"], data["b64"], lt=True)
    rho_lt, _ = ds.rows_rho(x, data["l64"], data["b64"], KAPPA, lt=True)
    assert rho_lt <= 1.0
    # ... and the rule is about THIS system: the solution of the other form does not pass
    assert ds.rows_rho(x, data["l64"], data["b64"], KAPPA)[0] >= 1e3


@pytest.mark.parametrize("tile", FACTOR_TILES, ids=lambda t: "p%d-I%d-J%d" % t)
@pytest.mark.parametrize("kind", ds.MUTATIONS)
def test_every_factor_mutant_is_caught(data, capsys, kind, tile):
    """One tile's update by one panel, mutated: FP64 rho >= 1e3 with the mutated tile named, FP32 forward error >= 80 x
    LAPACK's.  A factorisation that stops being positive definite counts as caught."""
    mutate = (kind,) + tile
    try:
        low = ds.blocked_cholesky(data["k64"], NB, mutate)
        rho, worst = ds.factor_rho(low, data["k64"], KAPPA)
    except np.linalg.LinAlgError:
        rho, worst = float("inf"), tile[1:]
    try:
        low32 = ds.blocked_cholesky(data["k32"], NB, mutate)
        ratio = ds.fp32_ratio(ds.forward_error(low32, data["l32_oracle"]), data["factor_ref_err"])
    except np.linalg.LinAlgError:
        ratio = float("inf")
    _say(capsys, "factor mutant %-17s panel %d tile (%d, %d): FP64 rho %.2e at tile %s, FP32 %.2e x LAPACK's"
         % ((kind,) + tile + (rho, worst, ratio)))
    assert rho >= 1e3
    assert worst == tile[1:]                     # the residual of a right-looking factorisation sits in the mutated tile
    assert ratio >= 10 * ds.FP32_MARGIN


@pytest.mark.parametrize("tile", ROWS_TILES, ids=lambda t: "p%d-J%d" % t)
@pytest.mark.parametrize("kind", ds.MUTATIONS)
def test_every_rows_mutant_is_caught(data, capsys, kind, tile):
    mutate = (kind,) + tile
    w = ds.rows_solve(data["l64"], data["b64"], NB, mutate)
    rho, worst = ds.rows_rho(w, data["l64"], data["b64"], KAPPA)
    w32 = ds.rows_solve(data["l32_lapack"], data["b32"], NB, mutate)
    ratio = ds.fp32_ratio(ds.forward_error(w32, data["w32_oracle"]), data["rows_ref_err"])
    _say(capsys, "rows mutant   %-17s panel %d column tile %d: FP64 rho %.2e at tile %s, FP32 %.2e x LAPACK's"
         % ((kind,) + tile + (rho, worst, ratio)))
    assert rho >= 1e3
    assert worst == (0, tile[1])
    assert ratio >= 10 * ds.FP32_MARGIN


@pytest.mark.parametrize("form,n,seed", ds.host_condition_sizes(), ids=lambda v: str(v))
def test_conditions_of_every_matrix_the_gpu_file_uses(capsys, form, n, seed):
    """Tile weight >= 1e-3 on the oracle's factor and cond(K) within its bound, for both forms, at the GPU file's sizes
    up to n = 6144 (the larger ones are asserted there, on the oracle's factor)."""
    if form == "lowrank":
        g = ds.lowrank_spd(n, seed)
        cond, bound = ds.lowrank_cond(g), ds.lowrank_cond_bound(n)
        k = ds.lowrank_matrix(g)
    else:
        x = ds.kernel_dense_points(n, seed)
        k = oracle.rbf_gram(x, None, ds.KERNEL_ELL, ds.KERNEL_SF2, ds.KERNEL_NOISE)
        # lambda_min >= noise (a Gram matrix plus noise I); lambda_max by Lanczos
        lam_max = float(spla.eigsh(k, k=1, which="LA", return_eigenvectors=False)[0])
        cond, bound = lam_max / ds.KERNEL_NOISE, ds.kernel_cond_bound(n)
    tw = ds.tile_weight(ds.factor(k))
    _say(capsys, "%s n = %d seed %d: cond %.4g (bound %.4g), tile weight %.2e" % (form, n, seed, cond, bound, tw))
    assert cond <= bound
    assert tw >= ds.MIN_TILE_WEIGHT


@pytest.mark.parametrize("tile", ROWS_TILES, ids=lambda t: "p%d-J%d" % t)
@pytest.mark.parametrize("kind", ds.MUTATIONS)
def test_kinv_diag_bound_sees_every_rows_mutant(data, capsys, kind, tile):
    """diag(K^-1) from rows of L^-T (the rows solve of the identity): the clean result sits far inside
    dense_spd.kinv_diag_bound and one mutated update moves it to at least 1e3 times the bound, so the derived bound, wide
    as it is beside the clean error, is not what would let a wrong tile through."""
    bound = ds.kinv_diag_bound(N, KAPPA)
    want = ds.kinv_diag(data["l64"])
    eye = np.eye(N)
    clean = ds.rows_solve(data["l64"], eye, NB)
    err_clean = ds.forward_error((clean * clean).sum(1), want)
    u = ds.rows_solve(data["l64"], eye, NB, (kind,) + tile)
    err = ds.forward_error((u * u).sum(1), want)
    _say(capsys, "kinv_diag mutant %-17s panel %d column tile %d: error %.2e, clean %.2e, bound %.2e" % ((kind,) + tile + (err, err_clean, bound)))
    assert err_clean <= bound
    assert err >= 1e3 * bound


def test_the_first_draw_is_taken_but_for_the_pinned_cases():
    """lowrank_spd rejects a draw that misses the cond bound: which matrices of the tables that changes is pinned."""
    got = {key: ds.lowrank_draws(*key)[1] for key in ds.lowrank_table()}
    assert {key: v for key, v in got.items() if v} == ds.REDRAWN


def test_term_by_term_accumulation_on_top_of_c_drifts_on_the_diagonal(capsys):
    """The cause of the FP32 finding, reproduced without the library (dense_spd.diagonal_by_order_f32) at n = 4096: the
    diagonal of L from K_jj minus the squares one at a time, against one subtraction per block of 256.  The first errs
    several times more, more the further right the column, and reads too large on average; the second stays at the
    rounding of a handful of operations."""
    n = 4096
    g = ds.lowrank_spd(n, n)
    k = ds.lowrank_matrix(g).astype(np.float32).astype(np.float64)
    low = ds.factor(k)
    seq, blk = ds.diagonal_by_order_f32(low, np.diag(k))
    exact = np.diag(low)
    scale = np.max(np.abs(low))
    e_seq, e_blk = (seq - exact) / scale, (blk - exact) / scale
    first, last = slice(0, n // 4), slice(3 * n // 4, n)
    _say(capsys, "diagonal of L in FP32 at n = %d: term by term max %.2e (first quarter %.2e, last quarter %.2e, mean %+.2e); "
         "per block max %.2e (mean %+.2e)" % (n, np.abs(e_seq).max(), np.abs(e_seq[first]).max(), np.abs(e_seq[last]).max(),
                                             e_seq.mean(), np.abs(e_blk).max(), e_blk.mean()))
    assert np.abs(e_seq).max() >= 3 * np.abs(e_blk).max()
    assert np.abs(e_seq[last]).max() >= 2 * np.abs(e_seq[first]).max()


def test_the_case_table_names_a_path_for_every_case():
    cases = ds.POTRF + ds.POTRF_ROWS + ds.BATCHED + ds.BLOCK_POSTERIOR + ds.STAGED + [ds.LAYER]
    assert all(isinstance(c[-1], str) and len(c[-1]) > 20 for c in cases)
    assert [c[0] for c in ds.POTRF] == [700, 5120, 5184, 5377, 6144, 8192, 9216, 10240]
