/* cimrgp_inducing.h -- greedy inducing-point selection: a matrix-free pivoted Cholesky factorisation of K(X, X), stopped
 * after m columns ("Greedy inducing-point selection").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h.  The covariance is
 *   k(x, x') = k_cov(x, x'; ell, sf2) + sum_e lin[e] x_e x'_e
 * with k_cov one of CIMRGP_COV_* and the linear term absent when lin_dev is NULL; ARD is the caller's x / l at ell = 1.
 * K is never formed: step j reads the j earlier columns of the factor and writes one.  FP64 only.
 *
 * Semantics.
 *   Start    d_i = k(x_i, x_i), formed directly as sf2 + sum_e lin[e] x_ie^2 (not through the covariance function: without a
 *            linear term every d_i is the same bits).  trace[0] = sum_i d_i.
 *   Pick     step j = 0 .. m - 1: p_j = the arg-max of d over the rows not yet picked, ties to the LOWEST row index; a NaN
 *            residual is never larger than anything.  pivots[j] = p_j.  The m pivots are m distinct valid rows whatever
 *            the data.
 *   Column   if d_p > floor: c_i = (k(x_i, x_p) - sum_{t < j} L_it L_pt) / sqrt(d_p) for EVERY row i (picked rows too),
 *            written as column j of L, and d_i -= c_i^2 for the rows not yet picked.  Otherwise column j is zero and d is
 *            unchanged.  Row p_j is then marked as picked and is never picked again.
 *   Trace    trace[j + 1] = sum over the rows not yet picked (after step j) of max(d_i, 0): tr(K - Q_j) of the VFE bound.
 *   Rank     rank[0] = the number of steps whose pivot residual exceeded floor.
 *
 * Layout.  lt_dev is m x ldl with ldl >= n: ROW j of lt_dev is COLUMN j of L, contiguous over i, so that the pass over the
 * earlier columns coalesces.  Columns >= n of a row and rows >= m are never touched.  diag_dev has n entries: the residual
 * of the rows not picked, and -1 for the picked rows.  trace_dev has m + 1 entries, pivots_dev m, rank_dev 1.
 *
 * Order.  Every sum is FP64 in a fixed order and there are no atomics: pivots, L, diag and trace are bit-identical from
 * run to run.  Row i's sum over the earlier columns is four partial sums, t = w, w + 4, .. ascending for w = 0 .. 3, added
 * as ((s0 + s1) + s2) + s3: a function of (i, j) alone.  The arg-max and the trace are taken per 64 rows (a butterfly
 * over the wave), then over those records by 256 threads (thread t takes records t, t + 256, ..) and a pairwise tree:
 * a function of n alone.  So the pivots and the trace of a run with m' < m are the first m' (+ 1) entries of the run with
 * m, bit for bit, and so are the first m' rows of lt_dev.
 *
 * The call is enqueue-only on `stream` (two plain launches per step, the pivot index stays in device memory between them;
 * nothing is read back) and checks all of its arguments before any device work. */
#ifndef CIMRGP_INDUCING_H
#define CIMRGP_INDUCING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of one arg-max / trace record (one wave of the column kernel). */
#define CIMRGP_PIVCHOL_ROWS 64

/* Bytes of scratch cimrgp_pivoted_cholesky needs: the pivot row's m earlier coefficients (float64), the picked marks (n
 * int32), one (value, trace, index) record per CIMRGP_PIVCHOL_ROWS rows and the pivot's (index, residual); each part
 * rounded up to 16 bytes.  0 for sizes outside 1 <= m <= n < 2^31. */
size_t cimrgp_pivoted_cholesky_scratch_bytes(int64_t n, int64_t m);

/* The factorisation above of the n rows of x_dev (n x d, row-major without padding, float64).  Requires dtype =
 * CIMRGP_F64 (CIMRGP_F32 is refused: not built -- the cancellation in the residual is what FP32 cannot hold), a known
 * cov, 1 <= m <= n < 2^31, d in [1, 8], ell > 0, sf2 > 0, a finite floor >= 0, ldl >= n, no null pointer except lin_dev,
 * a 16-byte aligned scratch_dev and scratch_bytes >= cimrgp_pivoted_cholesky_scratch_bytes(n, m).  Every output is
 * OVERWRITTEN; x_dev and lin_dev are only read. */
int cimrgp_pivoted_cholesky(int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2,
                            const double* lin_dev, int64_t m, double floor, int64_t* pivots_dev, void* lt_dev, int64_t ldl,
                            double* diag_dev, double* trace_dev, int64_t* rank_dev, void* scratch_dev, size_t scratch_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_INDUCING_H */
