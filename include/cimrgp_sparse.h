/* cimrgp_sparse.h -- the three device calls of inducing-point (sparse) GP regression that the dense path lacks
 * ("Sparse (inducing-point) GP regression").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, the 0 / <0 return convention and cimrgp_last_error
 * are defined there).  With n training inputs X, m inducing inputs Z, K_uu + eps sf I = L_u L_u^T and
 *   A = K(X, Z) L_u^-T   (n x m, row-major: cimrgp_cov_cross then cimrgp_trsm_rows)
 * the FITC / VFE posterior needs
 *   q_i = sum_j A_ij^2,  lambda_i = sf - q_i + noise (FITC) | noise (VFE),  w_i = 1 / lambda_i      cimrgp_sparse_lambda
 *   B = I + A^T diag(w) A  (m x m, lower),  c = A^T diag(w) r  (m x q)                               cimrgp_wsyrk_tn
 *   mean* = W* gamma,  var* = sf + extra - sum A*^2 + sum W*^2                                       cimrgp_sparse_tail
 * and otherwise the existing calls (cimrgp_cov_gram, cimrgp_cov_cross, cimrgp_potrf, cimrgp_trsm_rows, cimrgp_potrs,
 * cimrgp_logdet_half).  All calls take device pointers and a stream, are enqueue-only (no host read-back) and check
 * every argument before any device work (errors name the entry point). */
#ifndef CIMRGP_SPARSE_H
#define CIMRGP_SPARSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest m (columns of A) and n (rows of A) cimrgp_wsyrk_tn accepts. */
#define CIMRGP_WSYRK_MAX_M 16384
#define CIMRGP_WSYRK_MAX_N (1 << 24)

/* Bytes of scratch cimrgp_wsyrk_tn needs for an n x m operand and q right-hand sides (q = 0: no g): the partial
 * 128 x 128 tiles of the S(n, m) slices of K = n, and the slices' partial g.  0 for an unknown dtype or sizes outside
 * [1, CIMRGP_WSYRK_MAX_N] x [1, CIMRGP_WSYRK_MAX_M] x [0, 8]. */
size_t cimrgp_wsyrk_tn_scratch_bytes(int dtype, int64_t n, int64_t m, int q);

/* The weighted transposed rank-n product on the matrix cores:
 *   lower(C)[i][j] = diag_add [i = j] + sum_k w[k] A[k][i] A[k][j]        (i, j < m, j <= i; k < n)
 *   g[i][c]        =                    sum_k w[k] A[k][i] r[k][c]        (m x q, row-major; only if r_dev != NULL)
 * A is n x m row-major with pitch lda, w has n elements, r is n x q row-major (q in [1, 8]; q is ignored and g_dev may
 * be NULL when r_dev is NULL).  Both sums are taken in the same pass: A is read once per output tile column.
 * K = n is cut into S slices (S depends on n and m alone); every slice writes its partial tiles to scratch_dev, and a
 * second kernel adds the S partials in slice order: no atomics, the result is bit-identical from run to run and does
 * not depend on what else runs on the device.
 * Memory: only the lower triangle of C (j <= i) is written; columns >= m of A (lda > m) and rows >= n of A, w and r
 * are never read.  Requires 1 <= n <= CIMRGP_WSYRK_MAX_N, 1 <= m <= CIMRGP_WSYRK_MAX_M, lda >= m, ldc >= m, lda a
 * multiple of 16 bytes, 16-byte aligned a_dev and scratch_dev, scratch_bytes >= cimrgp_wsyrk_tn_scratch_bytes. */
int cimrgp_wsyrk_tn(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* w_dev, const void* r_dev,
                    int q, double diag_add, void* c_dev, int64_t ldc, void* g_dev, void* scratch_dev, size_t scratch_bytes,
                    void* stream);

/* One pass over A (n x m, pitch lda): q_i = sum_j A_ij^2 (FP64 accumulation, fixed order),
 *   mode 0 (FITC): lam[i] = sf2 - q_i + noise        mode 1 (VFE / DTC): lam[i] = noise
 *   w[i] = 1 / lam[i]
 *   sums[0] = sum_i log lam[i],  sums[1] = sum_i (sf2 - q_i),  sums[2] = the number of i with lam[i] <= 0 (or NaN)
 * sums_dev: 3 doubles, summed in a fixed order.  lam_dev and w_dev: n elements each.  Columns >= m and rows >= n of A
 * are never read.  n >= 1, 1 <= m, lda >= m. */
int cimrgp_sparse_lambda(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, double sf2, double noise, int mode,
                         void* lam_dev, void* w_dev, double* sums_dev, void* stream);

/* The predictive tail of ns test points: A* and W* = A* L_B^-T (ns x m each, pitch lda), gamma (m x q, row-major):
 *   mean[i][c] (+)= sum_j W*[i][j] gamma[j][c]                                  (ns x q; needs wstar, gamma, q in [1, 8])
 *   var[i]     (+)= sf2 + extra_var - sum_j A*[i][j]^2 + sum_j W*[i][j]^2       (ns; needs astar and wstar)
 * Either output may be NULL (both: nothing is done); accumulate != 0 adds to what the outputs hold.  Sums are taken in
 * FP64 in a fixed order; a row's result does not depend on ns. */
int cimrgp_sparse_tail(int dtype, const void* astar_dev, const void* wstar_dev, int64_t ns, int64_t m, int64_t lda,
                       const void* gamma_dev, int q, double sf2, double extra_var, void* mean_dev, void* var_dev,
                       int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_H */
