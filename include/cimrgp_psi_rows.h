/* cimrgp_psi_rows.h -- one row's own Psi2, contracted with weights and never stored: what the predictive variance at an
 * uncertain test input needs ("Predictive variance at uncertain test inputs").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h.  Notation, operands and conventions are those of
 * cimrgp_psi.h: x_i ~ N(mu_i, diag s_i), inducing inputs z_j, variance sf2, length-scales l_e (ell_dev, float64 on the
 * device); mu and s are n x d, z is m x d, row-major without padding and of the call's dtype.  Row i's own term of Psi2 is
 *   Psi2_i[j][k] = E k(z_j, x_i) k(x_i, z_k) = sf2^2 exp(-delta_jk - t_ijk)
 *   delta_jk = sum_e (z_je - z_ke)^2 / (4 l_e^2)
 *   t_ijk    = 1/2 sum_e log1p(2 s_ie / l_e^2) + sum_e (mu_ie - (z_je + z_ke) / 2)^2 / (l_e^2 + 2 s_ie)
 * (cimrgp_psi2 returns its sum over the rows).  Every call is enqueue-only on `stream` and checks all of its arguments
 * before any device work.  Requires d in [1, 8], q in [1, 8], sf2 > 0, 1 <= n <= CIMRGP_PSI2_MAX_N,
 * 1 <= m <= CIMRGP_PSI2_MAX_M. */
#ifndef CIMRGP_PSI_ROWS_H
#define CIMRGP_PSI_ROWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The grouping of cimrgp_psi2_rows_quad: a function of m alone.  The lower triangle of the m x m pairs is cut into the
 * tiles of cimrgp_psi.h (CIMRGP_PSI2_TILE x CIMRGP_PSI2_TILE pairs, t = ceil(m / TILE) per side, T = t (t + 1) / 2 in all,
 * in cimrgp_psi2's tile order); the tile list into groups of consecutive tiles so that there are at most
 * CIMRGP_PSI_ROWS_GROUPS of them:
 *   g = ceil(T / CIMRGP_PSI_ROWS_GROUPS) tiles per group        G = ceil(T / g) groups
 * Group p holds tiles [p g, min(T, (p + 1) g)).  A row's sums are taken pair by pair in tile order within a group (a
 * tile's pairs row by row, k ascending), and the G subtotals are added in group order: the order depends on (m, d, q)
 * alone, so a row's results depend on that row's data and on (m, d, q) and not on n or on where the row lies in the
 * operands. */
#define CIMRGP_PSI_ROWS_GROUPS 16

/* Bytes of scratch cimrgp_psi2_rows_quad needs: one count per 256 rows (float64), the rows' 2 d + 1 constants, and the G
 * subtotals of every row's 1 + q sums (G n (1 + q) of the dtype); each part rounded up to 16 bytes.  0 for an unknown
 * dtype or sizes outside the limits. */
size_t cimrgp_psi2_rows_quad_scratch_bytes(int dtype, int64_t n, int64_t m, int d, int q);

/* For every row i < n, with a SYMMETRIC c_dev (m x m, pitch ldc >= m) of which only [j][k] with k <= j is read (an
 * off-diagonal pair stands for both (j, k) and (k, j)) and a_dev (m x q, row-major, pitch lda >= q):
 *   tr[i]      = sum_jk c[j][k] Psi2_i[j][k]              over the full square          (tr_dev, n)
 *   quad[i][c] = sum_jk a[j][c] a[k][c] Psi2_i[j][k]      = a_c^T Psi2_i a_c, c < q     (quad_dev, n x q, pitch ldq >= q)
 * Three kernels:
 *   1. cimrgp_psi2's pass over the rows: each row's constants mu_ie, 1 / (l_e^2 + 2 s_ie) and -1/2 sum_e log1p(2 s_ie /
 *      l_e^2) (formed in float64, rounded once to the dtype).  A row with a negative or non-finite variance is counted
 *      and given (0, 0, -infinity).
 *   2. one workgroup per (256 rows, group of tiles), a thread per row.  Per tile, staged in LDS: z / 2 of the tile's
 *      points, its rows of a, and the weights w sf2^2 exp(-delta_jk) and w c[j][k] sf2^2 exp(-delta_jk) (w = 1 on the
 *      diagonal, 2 off it).  Per (row, pair): the exponent in cimrgp_psi2's direct form, ONE exponential, one
 *      multiply-add for tr and one per output for sum_{k <= j} a[k][c] p_jk, which a[j][c] multiplies once per j.  The
 *      1 + q running sums stay in registers; the (row, group) subtotals go to scratch.
 *   3. the subtotals are added in group order; the counts of bad rows are added as cimrgp_psi2 adds them.
 * No atomics: two calls give the same bits.  Every output is OVERWRITTEN.  bad_dev[0] receives (is overwritten with) the
 * number of rows with a negative or non-finite variance; the outputs of such a row are zeros.  There is no division by
 * s: s_ie = 0 is exact, and then Psi2_i[j][k] = k(z_j, mu_i) k(mu_i, z_k).  Rows >= n of mu, s, tr and quad, rows >= m of
 * z, c and a, columns >= m of c, columns >= q of a and quad and the strict upper triangle of c are never read or written.
 * Requires ldc >= m, lda >= q, ldq >= q, a 16-byte aligned scratch_dev and
 * scratch_bytes >= cimrgp_psi2_rows_quad_scratch_bytes(dtype, n, m, d, q). */
int cimrgp_psi2_rows_quad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                          const double* ell_dev, double sf2, const void* c_dev, int64_t ldc, const void* a_dev, int64_t lda,
                          int q, void* tr_dev, void* quad_dev, int64_t ldq, void* scratch_dev, size_t scratch_bytes,
                          double* bad_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_PSI_ROWS_H */
