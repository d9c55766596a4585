/* cimrgp_psi.h -- the psi statistics of the RBF covariance under Gaussian inputs: what sparse GP regression on
 * uncertain inputs needs beside the calls of cimrgp_sparse.h ("Sparse GP regression on uncertain inputs").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, the 0 / <0 return convention and cimrgp_last_error
 * are defined there).  With inputs x_i ~ N(mu_i, diag s_i), s_ie >= 0 (i < n), inducing inputs z_j (j < m), the RBF
 * covariance of variance sf2 and length-scales l_e (e < d):
 *   Psi1[i][j] = E k(x_i, z_j)
 *              = sf2 exp( -1/2 sum_e [ log1p(s_ie / l_e^2) + (mu_ie - z_je)^2 / (l_e^2 + s_ie) ] )
 *   Psi2[j][k] = sum_i E k(z_j, x_i) k(x_i, z_k)
 *              = sf2^2 exp( -sum_e (z_je - z_ke)^2 / (4 l_e^2) )
 *                sum_i exp( -1/2 sum_e log1p(2 s_ie / l_e^2) - sum_e (mu_ie - (z_je + z_ke) / 2)^2 / (l_e^2 + 2 s_ie) )
 * At s = 0 they are K(mu, Z) and K(Z, mu) K(mu, Z).  mu and s are n x d, z is m x d, all row-major without padding and
 * of the call's dtype; ell_dev holds the d length-scales as float64 on the device (an isotropic caller passes d equal
 * values).  Every call is enqueue-only on `stream`, checks all of its arguments before any device work and names itself
 * in errors.  Requires d in [1, 8] and sf2 > 0. */
#ifndef CIMRGP_PSI_H
#define CIMRGP_PSI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Psi1 into out_dev (n x m, pitch ldo >= m).  A wave per row i: the row's d + 1 constants once, then lane l writes
 * columns l, l + 64, ..: ONE exponential per entry, no division by s (s_ie = 0 is exact: the entry is then k(mu_i, z_j)
 * up to rounding).  A row's values do not depend on n or on where the row lies in the operands.  A row with a negative
 * or non-finite variance holds unspecified values (cimrgp_psi2 counts such rows).  Rows >= n of mu and s and rows >= m
 * of z are never read; columns >= m of out are never written.  n = 0: nothing is done.
 * Requires 0 <= n < 2^31, 1 <= m < 2^31. */
int cimrgp_psi1(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                const double* ell_dev, double sf2, void* out_dev, int64_t ldo, void* stream);

/* The slicing of cimrgp_psi2: a function of n and m alone.  The lower triangle of Psi2 is cut into tiles of
 * CIMRGP_PSI2_TILE x CIMRGP_PSI2_TILE pairs, t = ceil(m / TILE) per side, t (t + 1) / 2 in all; the n rows into S
 * slices so that tiles x S is about CIMRGP_PSI2_TARGET_WGS workgroups and no slice is shorter than
 * CIMRGP_PSI2_MIN_SLICE rows:
 *   S0  = max(1, min(TARGET_WGS / tiles, ceil(n / MIN_SLICE)))
 *   len = ceil(n / S0) rounded up to a multiple of CIMRGP_PSI2_SLICE_ALIGN
 *   S   = ceil(n / len)                                                  = cimrgp_psi2_slices(n, m)
 * Slice s holds rows [s len, min(n, (s + 1) len)).  cimrgp_psi2_slices returns 0 for sizes outside the limits below. */
#define CIMRGP_PSI2_TILE 64
#define CIMRGP_PSI2_TARGET_WGS 2048
#define CIMRGP_PSI2_MIN_SLICE 64
#define CIMRGP_PSI2_SLICE_ALIGN 16
/* Largest m and n cimrgp_psi2 accepts (those of cimrgp_wsyrk_tn). */
#define CIMRGP_PSI2_MAX_M 16384
#define CIMRGP_PSI2_MAX_N (1 << 24)
int cimrgp_psi2_slices(int64_t n, int64_t m);

/* Bytes of scratch cimrgp_psi2 needs: one count per 256 rows (float64), the rows' 2 d + 1 constants, and the S partial
 * tiles of every tile of the lower triangle.  0 for an unknown dtype or sizes outside [1, CIMRGP_PSI2_MAX_N] x
 * [1, CIMRGP_PSI2_MAX_M] x [1, 8]. */
size_t cimrgp_psi2_scratch_bytes(int dtype, int64_t n, int64_t m, int d);

/* The lower triangle of Psi2 into c_dev (m x m, pitch ldc >= m): only [j][k] with k <= j is written.  Three kernels:
 *   1. a pass over the rows writes each row's constants: mu_ie, 1 / (l_e^2 + 2 s_ie) and -1/2 sum_e log1p(2 s_ie / l_e^2)
 *      (formed in float64, rounded once to the dtype).  A row with a negative or non-finite variance is counted and
 *      given the constants (0, 0, -infinity): its exponential is exactly 0 and it adds nothing.
 *   2. one workgroup per (tile, slice): a thread owns 4 x 4 pairs, z_j / 2 and z_k / 2 in registers, the slice's row
 *      constants staged through LDS; per (row, pair) d subtract-multiply-adds in the direct form
 *      (mu - (z_j + z_k) / 2)^2 / (l^2 + 2 s) and ONE exponential.  The partial tile goes to scratch.
 *   3. the partial tiles are added in slice order and multiplied by sf2^2 exp(-sum_e (z_je - z_ke)^2 / (4 l_e^2)).
 * No atomics: the result is bit-identical from run to run and does not depend on what else runs on the device.
 * bad_dev[0] receives (is overwritten with) the number of rows with a negative or non-finite variance.
 * Rows >= n of mu and s and rows >= m of z are never read.
 * Requires 1 <= n <= CIMRGP_PSI2_MAX_N, 1 <= m <= CIMRGP_PSI2_MAX_M, ldc >= m, a 16-byte aligned scratch_dev and
 * scratch_bytes >= cimrgp_psi2_scratch_bytes(dtype, n, m, d). */
int cimrgp_psi2(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                const double* ell_dev, double sf2, void* c_dev, int64_t ldc, void* scratch_dev, size_t scratch_bytes,
                double* bad_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_PSI_H */
