/* cimrgp_grad.h -- derivatives of the dense block posterior with respect to the test inputs (GPy's
 * GP.predictive_gradients): d mean / d x* and d var / d x*.
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, CIMRGP_COV_*, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  For one block with training inputs X (n x d), factor K = L L^T (noise
 * included), weights alpha = K^-1 r (n x q) and a test point x* with k* = k(x*, X):
 *   d mean_c / d x*_e = sum_j alpha[j][c] dk(x*, x_j)/dx*_e
 *   d var    / d x*_e = -2 sum_j beta[j] dk(x*, x_j)/dx*_e,     beta = K^-1 k* = L^-T (L^-1 k*)
 * and every covariance of the dense path has dk/dx*_e = -g(r) (x*_e - x_je), r = |x* - x_j| ("Predictive
 * gradients"):
 *   RBF        g = sf2 / ell^2 exp(-r^2 / (2 ell^2))
 *   MATERN12   g = sf2 / (ell r) exp(-r / ell),  taken as 0 at r = 0 (GPy's convention: no derivative there)
 *   MATERN32   g = 3 sf2 / ell^2 exp(-sqrt(3) r / ell)
 *   MATERN52   g = 5 sf2 / (3 ell^2) (1 + sqrt(5) r / ell) exp(-sqrt(5) r / ell)
 * All calls take device pointers and a stream, are enqueue-only (no host read-back) and check every argument before
 * any device work (errors name the entry point). */
#ifndef CIMRGP_GRAD_H
#define CIMRGP_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Row-wise backward triangular solve, the mirror of cimrgp_trsm_rows:
 *   B <- B L^-1      B: (m x n) row-major, ldb >= n,  i.e. row i of B becomes L^-T b_i.
 * After cimrgp_trsm_rows on B = K(X*, X) this gives the rows of K(X*, X) K^-1.  l_dev and workspace_dev are a factor
 * and its workspace from cimrgp_potrf (or any call that leaves the same workspace); the inverted 256 x 256 diagonal
 * blocks are read from it.  Panels of 256 columns are swept from the last to the first:
 *   B_p <- B_p inv(L_pp);   B_{<p} -= B_p L[p, <p]
 * both on the matrix cores.  Any n >= 1 (a ragged last panel included).  Only the columns [0, n) of the m rows of B
 * are read or written.  Requires ldl >= n, ldb >= n, leading dimensions that are multiples of 16 bytes and 16-byte
 * aligned l_dev, workspace_dev and b_dev. */
int cimrgp_trsm_rows_lt(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* b_dev,
                        int64_t m, int64_t ldb, void* stream);

/* The same for `batch` equal-sized factors in the same launches: factor b at l_dev + b * l_stride (elements), its
 * workspace at workspace_dev + b * workspace_stride_bytes, its rows at b_dev + b * b_stride (elements); the layout of
 * the arenas of cimrgp_layer_predict.  Requires, besides the above, workspace_stride_bytes >=
 * cimrgp_potrf_workspace_bytes(dtype, n), strides that are multiples of 16 bytes and, for batch > 1, strides that do
 * not make the blocks of B overlap. */
int cimrgp_trsm_rows_lt_batched(int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride,
                                const void* workspace_dev, size_t workspace_stride_bytes, void* b_dev, int64_t m,
                                int64_t ldb, int64_t b_stride, int batch, void* stream);

/* The fused derivative contraction of one block (the cross-covariance and its derivative are never stored):
 *   mean_grad[i][e][c] (+)= sum_j alpha[j][c] (-g_ij) (xs[i][e] - x[j][e])      (ns x d x q), if mean_grad_dev
 *   var_grad[i][e]     (+)= 2 sum_j beta[i][j] g_ij (xs[i][e] - x[j][e])        (ns x d),     if var_grad_dev
 * with g_ij = g(|xs_i - x_j|) of covariance `cov` (above), beta (ns rows of ldb >= n) the rows of K(X*, X) K^-1
 * (cimrgp_trsm_rows, then cimrgp_trsm_rows_lt).  accumulate != 0 adds to the outputs.  Either output may be NULL (both:
 * nothing is done); alpha_dev is required with mean_grad_dev, beta_dev with var_grad_dev.  Requires n >= 1, ns >= 0,
 * d in [1, 8], q in [1, 8], ell > 0, sf2 > 0. */
int cimrgp_cov_predict_grad(int dtype, int cov, const void* x_dev, int64_t n, int d, const void* alpha_dev, int q,
                            const void* xs_dev, int64_t ns, double ell, double sf2, const void* beta_dev, int64_t ldb,
                            void* mean_grad_dev, void* var_grad_dev, int accumulate, void* stream);

/* The batched counterpart of cimrgp_layer_predict_cov: for each of `batch` blocks of one layer (training side as there:
 * x, starts, n, cov, ell, sf2, the factors L_b and their workspaces) at its ns test points (rows t_starts_dev[b] .. + ns
 * of xs):
 *   W_b = K(xs_b, x_b) L_b^-T       (matrix b of w_arena_dev: ns x ldw, stride w_stride; a work area)
 *   beta_b = W_b L_b^-1             (in place: cimrgp_trsm_rows_lt_batched)
 *   mean_grad[t_b + i] (+)= ..., var_grad[t_b + i] (+)= ...   as cimrgp_cov_predict_grad with alpha_b, beta_b
 * alpha_dev: batch blocks of (n x q), block b at alpha_dev + b n q.  mean_grad_dev (N* x d x q) and var_grad_dev
 * (N* x d) are shared by the blocks (they must write disjoint test ranges) and either may be NULL; without
 * var_grad_dev, W is neither formed nor read and w_arena_dev may be NULL.  Requires n >= 1, ns >= 0 (0: nothing is
 * done), d in [1, 8], q in [1, 8], ell > 0, sf2 > 0, ldl >= n, ldw >= n, leading dimensions and strides that are
 * multiples of 16 bytes, 16-byte aligned arenas and, for batch > 1, strides that do not make blocks overlap. */
int cimrgp_layer_predict_grad_cov(int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d,
                                  const void* xs_dev, const int64_t* t_starts_dev, int64_t ns, int batch, double ell,
                                  double sf2, const void* l_arena_dev, int64_t ldl, int64_t l_stride,
                                  const void* ws_arena_dev, size_t ws_stride_bytes, const void* alpha_dev, int q,
                                  void* w_arena_dev, int64_t ldw, int64_t w_stride, void* mean_grad_dev,
                                  void* var_grad_dev, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_GRAD_H */
