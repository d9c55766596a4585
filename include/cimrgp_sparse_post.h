/* cimrgp_sparse_post.h -- posterior queries of the sparse (inducing-point) GP after a fit: predictive gradients, the
 * leave-one-out prediction and the joint predictive covariance ("Posterior queries of the sparse GP").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, covariance ids, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  Notation of cimrgp_sparse.h: A* = K(X*, Z) L_u^-T, W* = A* L_B^-T, gamma (m x q).
 * Every call is enqueue-only on `stream`, checks all of its arguments before any device work and names itself in errors.
 * Matrices are row-major. */
#ifndef CIMRGP_SPARSE_POST_H
#define CIMRGP_SPARSE_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The cross-covariance and its d derivative slabs w.r.t. the ROW points in one pass over the pairs (xa_i, xb_j):
 *   slab 0      [i][j] = k(xa_i, xb_j)
 *   slab e + 1  [i][j] = dk(xa_i, xb_j) / d xa_ie = -g(r_ij) (xa_ie - xb_je)          e = 0 .. d - 1
 * with g of cimrgp_grad.h (0 at r = 0 for Matern 1/2); a pair's exponential is evaluated once for k and g.  Slab s is
 * the na x nb matrix of pitch ldo at out_dev + s * slab_stride (elements).  Slab 0 is bit-identical to what
 * cimrgp_cov_cross writes for the same arguments.  Columns >= nb and rows >= na of a slab are never written; xa rows
 * >= na and xb rows >= nb are never read.  na = 0 or nb = 0: nothing is done.
 * Requires d in [1, 8], ell > 0, sf2 > 0, ldo >= nb, slab_stride >= (na - 1) ldo + nb, na, nb < 2^30. */
int cimrgp_cov_cross_grad(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, double ell,
                          double sf2, void* out_dev, int64_t ldo, int64_t slab_stride, void* stream);

/* The predictive gradients from the solved slabs: a_dev holds the d + 1 slabs [A*; dA_0; ..] (cimrgp_cov_cross_grad's
 * output after cimrgp_trsm_rows against L_u), w_dev the same slabs after the second solve against L_B, both ns x m of
 * pitch ld at `slab_stride` elements apart.
 *   mean_grad[i][e][c] (+)= sum_j dW_e[i][j] gamma[j][c]                               (ns x d x q)
 *   var_grad[i][e]     (+)= 2 sum_j (W*[i][j] dW_e[i][j] - A*[i][j] dA_e[i][j])        (ns x d)
 * Either output may be NULL (both: nothing is done); a_dev may be NULL without var_grad, gamma_dev without mean_grad.
 * accumulate != 0 adds to what the outputs hold.  One wave per (row, e): lane l adds columns l, l + 64, .. in FP64, then
 * the 64 partial sums are added pairwise -- a fixed order, so a row's result does not depend on ns or on where the row
 * lies in the operand; one rounding to the dtype at the end.  Columns >= m and rows >= ns are never read. */
int cimrgp_sparse_tail_grad(int dtype, const void* a_dev, const void* w_dev, int64_t ns, int64_t m, int d, int64_t ld,
                            int64_t slab_stride, const void* gamma_dev, int q, void* mean_grad_dev, void* var_grad_dev,
                            int accumulate, void* stream);

/* Leave-one-out prediction of the rows of a sparse fit from A (n x m, rows of K(X, Z) L_u^-T) and V = A L_B^-T (same
 * shape and pitch), gamma (m x q) and the fit's targets r (n x q): per row i
 *   q_i = sum_j A_ij^2, lambda_i = sf2 - q_i + noise (mode 0, FITC) | noise (mode 1, VFE),
 *   h_i = sum_j V_ij^2 / lambda_i, mu_ic = sum_j V_ij gamma_jc,
 *   loo_mean[i][c] = r_ic - (r_ic - mu_ic) / (1 - h_i),   loo_var[i] = lambda_i / (1 - h_i)
 * (exact for the covariance A A^T + Lambda; the variance is that of an observation).  A row whose 1 - h_i is not
 * positive (or is NaN) adds 1 to *bad_dev, which the call never resets: it accumulates over the calls of a chunked
 * pass.  loo_mean_dev or loo_var_dev may be NULL.  Sums as in cimrgp_sparse_tail_grad (FP64, fixed order, a row's result
 * does not depend on n).  Columns >= m and rows >= n are never read.  n = 0: nothing is done. */
int cimrgp_sparse_loo(int dtype, const void* a_dev, const void* v_dev, int64_t n, int64_t m, int64_t ld, const void* gamma_dev,
                      const void* r_dev, int q, double sf2, double noise, int mode, void* loo_mean_dev, void* loo_var_dev,
                      int32_t* bad_dev, void* stream);

/* The joint predictive covariance of ns test points from their solved rows:
 *   lower(C) = K(xs, xs) + diag I - A* A*^T + W* W*^T
 * for astar_dev and wstar_dev (ns x m, pitch ld).  The Gram tiles are cimrgp_cov_gram's, the subtraction is
 * cimrgp_syrk_lower's update, the addition the same matrix-core tile body with a positive sign.  With cws_dev (a
 * factorisation workspace of cws_bytes >= cimrgp_potrf_workspace_bytes(dtype, ns)) C is then factored in place,
 * *info_dev receives cimrgp_potrf's status, and the strict upper triangle of the ns x ns block is set to zero: what
 * cimrgp_layer_joint_cov does for a batch of one, ready for cimrgp_layer_sample.  What the strict upper triangle of C
 * holds on entry is never used; without cws_dev the call may leave covariance values there inside the tiles that hold
 * the diagonal (as cimrgp_cov_gram's lower_only and cimrgp_syrk_lower do), nothing else.  A 16-byte chunk or a
 * 128-byte stage of a row of A* / W* may be loaded beyond column m within the pitch; what it holds there is masked and
 * never used.  ns = 0: nothing is done.
 * Requires d in [1, 8], ell > 0, sf2 > 0, 1 <= m < 2^31, ns < 2^30, ld >= m, ldc >= ns, ld and ldc multiples of 16
 * bytes, ld at least 128 bytes, all matrix pointers 16-byte aligned. */
int cimrgp_sparse_joint_cov(int dtype, int cov, const void* xs_dev, int64_t ns, int d, double ell, double sf2, double diag,
                            const void* astar_dev, const void* wstar_dev, int64_t m, int64_t ld, void* c_dev, int64_t ldc,
                            void* cws_dev, size_t cws_bytes, int32_t* info_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_POST_H */
