/* cimrgp_sparse_grad.h -- the device calls behind the analytic gradient of the sparse (inducing-point) objective with
 * respect to the hyper-parameters and the inducing inputs ("Gradients of the sparse objective").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, covariance ids, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  Notation of cimrgp_sparse.h, and with V = A L_B^-T, Y = V L_B^-1 (n x m),
 * b = L_B^-T gamma (m x q):
 *   beta_i = w_i (r_i - V_i gamma),  s_i = w_i - w_i^2 |V_i|^2,  h_i = (|beta_i|^2 - q s_i) / 2
 *   t_i = h_i (FITC)  |  -q / (2 noise) (VFE)                                                  cimrgp_sparse_grad_rows
 *   G_A = beta b^T - q diag(w) Y - 2 diag(t) A        (n x m, = dF / dA with B's dependence on A) cimrgp_sparse_grad_combine
 *   sums of G o K, G o dK/dlog l and db = sum_i G_ij dk(xa_i, xb_j)/dxb_j                         cimrgp_cov_pair_grad
 * and otherwise the existing calls (cimrgp_trsm_rows, cimrgp_trsm_rows_lt, cimrgp_wsyrk_tn).  All calls take device
 * pointers and a stream, are enqueue-only (no host read-back) and check every argument before any device work (errors
 * name the entry point). */
#ifndef CIMRGP_SPARSE_GRAD_H
#define CIMRGP_SPARSE_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest na (rows of G) and nb (columns of G) cimrgp_cov_pair_grad accepts. */
#define CIMRGP_PAIR_GRAD_MAX_NA (1 << 24)
#define CIMRGP_PAIR_GRAD_MAX_NB (1 << 20)

/* Bytes of scratch cimrgp_cov_pair_grad needs for an na x nb weight matrix and input dimension d: per slice and column
 * tile of 128 columns, 128 d partial sums of db and the two partial scalar sums, all FP64 (the same for both dtypes).
 * 0 for sizes outside [1, CIMRGP_PAIR_GRAD_MAX_NA] x [1, CIMRGP_PAIR_GRAD_MAX_NB] x [1, 8]. */
size_t cimrgp_cov_pair_grad_scratch_bytes(int64_t na, int64_t nb, int d);

/* The contraction of a weight matrix G (na x nb, row-major, pitch ldg) with the covariance of the pairs (xa_i, xb_j)
 * (xa: na x d, xb: nb x d, row-major, d in [1, 8]) and its derivatives, none of which is stored:
 *   sums[0] (+)= sum_ij G_ij k(xa_i, xb_j)
 *   sums[1] (+)= sum_ij G_ij (dk / dlog l)(xa_i, xb_j)                        dk/dlog l = -r dk/dr
 *   db[j][e] (+)= scale sum_i G_ij g(r_ij) (xa_ie - xb_je)                    (nb x d, row-major)
 * with dk(a, b)/da_e = -g(r) (a_e - b_e), so that the sum in db is d/dxb_je of sum_i G_ij k(xa_i, xb_j); g of
 * Matern 1/2 is taken as 0 at r = 0 (cimrgp_grad.h).  sums_dev (2 doubles) or db_dev may be NULL (both: nothing is
 * done); accumulate != 0 adds to what both outputs hold; scale multiplies the db sum only.
 * k, g and dk/dlog l are evaluated per pair in the dtype, as cimrgp_cov_cross evaluates k; the products with G and all
 * sums are FP64.  The rows are cut into S slices (S depends on na and nb alone); every workgroup -- one slice of one
 * tile of 128 columns -- writes its partial sums to scratch_dev, and a second kernel adds the partials in slice (and
 * tile) order: no atomics, the result is bit-identical from run to run and does not depend on what else runs on the
 * device.  G is read once; columns >= nb of G (ldg > nb) and rows >= na of G and xa are never read.
 * Requires 1 <= na <= CIMRGP_PAIR_GRAD_MAX_NA, 1 <= nb <= CIMRGP_PAIR_GRAD_MAX_NB, ldg >= nb, ell > 0, sf2 > 0,
 * scratch_bytes >= cimrgp_cov_pair_grad_scratch_bytes(na, nb, d). */
int cimrgp_cov_pair_grad(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d,
                         const void* g_dev, int64_t ldg, double ell, double sf2, double scale, int accumulate,
                         double* sums_dev, void* db_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* One pass over V = A L_B^-T (n x m, pitch ldv) with gamma (m x q), r (n x q), w (n), q in [1, 8]:
 *   beta[i][c] = w_i (r_ic - sum_j V_ij gamma_jc)                                 (n x q, row-major)
 *   h_i = (sum_c beta_ic^2 - q (w_i - w_i^2 sum_j V_ij^2)) / 2
 *   t[i] = h_i (mode 0, FITC)  |  -q / (2 noise) (mode 1, VFE / DTC)             (n)
 *   sums[0] = sum_i h_i,  sums[1] = sum_i t[i]                                   (2 doubles)
 * Row sums are taken in FP64 in a fixed order (a wave per row), the two sums over i likewise (over the h_i and t_i as
 * stored in the dtype).  Columns >= m and rows >= n of V are never read.  n >= 1, m >= 1, ldv >= m, noise > 0. */
int cimrgp_sparse_grad_rows(int dtype, const void* v_dev, int64_t n, int64_t m, int64_t ldv, const void* gamma_dev,
                            const void* r_dev, const void* w_dev, int q, int mode, double noise, void* beta_dev, void* t_dev,
                            double* sums_dev, void* stream);

/* In place on Y (n x m, pitch ldy), with A (n x m, pitch lda), beta (n x q), b (m x q), w and t (n):
 *   Y[i][j] <- sum_c beta_ic b_jc - q w_i Y[i][j] - 2 t_i A[i][j]
 * evaluated in FP64 and rounded once.  A and Y are read once each; columns >= m and rows >= n of either are neither
 * read nor written.  n >= 1, m >= 1, lda >= m, ldy >= m, q in [1, 8]. */
int cimrgp_sparse_grad_combine(int dtype, const void* a_dev, int64_t lda, void* y_dev, int64_t ldy, int64_t n, int64_t m,
                               const void* beta_dev, const void* b_dev, const void* w_dev, const void* t_dev, int q,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_GRAD_H */
