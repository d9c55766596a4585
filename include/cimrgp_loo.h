/* cimrgp_loo.h -- leave-one-out cross-validation of a fitted dense block (Rasmussen & Williams 5.4.2) and the
 * triangular inverse behind it.
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, the 0 / <0 return convention and cimrgp_last_error
 * are defined there).  For one block with K = L L^T (noise included), targets y, weights alpha = K^-1 r (n x q) and
 *   d_i = [K^-1]_ii = sum_k (L^-1)_ki^2 = |row i of L^-T|^2
 * the prediction of y_i from the other n - 1 points of the block is closed form ("Leave-one-out
 * cross-validation"):
 *   loo_mean[i][c] = y[i][c] - alpha[i][c] / d_i          loo_var[i] = 1 / d_i   (noise included, shared by the outputs)
 * Everything but d is resident after a fit; d comes from row strips of U = L^-T (upper triangular), each reduced to
 * its rows' sums of squares: n^3 / 3 flop and O(n x strip) memory, against n^3 flop and an n x n buffer for the
 * identity carried through cimrgp_trsm_rows.
 * All calls take device pointers and a stream, are enqueue-only (no host read-back) and check every argument before
 * any device work (errors name the entry point). */
#ifndef CIMRGP_LOO_H
#define CIMRGP_LOO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Rows [r0, r0 + m) of U = L^-T into u_dev (m x ldu, row i of u_dev = row r0 + i of U, columns indexed as in U):
 * the forward row solve B <- B L^-T of cimrgp_trsm_rows applied to rows of the identity, without the work that is
 * structurally zero: row i of U has no entry left of column i, so the sweep over the 256-column panels starts at
 * panel r0 / 256 and a row joins the sweep at its own panel:
 *   per panel p >= r0 / 256:   U[rows <= p, p] <- U[rows <= p, p] L_pp^-T          (the stored inverse, 32-row strips)
 *                              U[rows <= p, > p] -= U[rows <= p, p] L[> p, p]^T    (matrix-core tiles, K = 256)
 * l_dev and workspace_dev are a factor and its workspace from cimrgp_potrf (or any call that leaves the same
 * workspace); the inverted 256 x 256 diagonal blocks are read from it, the strict upper triangle of L never is.
 * r0 must be a multiple of 256, r0 + m <= n; any n >= 1 (a ragged last panel and a ragged m included).  Columns
 * [r0, n) of the m rows are written (zeros left of the diagonal); columns left of r0 are neither read nor written.
 * With r0 = 0 and m = n this is the whole triangular inverse.  Every row of U is its own chain of products in a fixed
 * order: its bits do not depend on r0 or m.  Requires ldl >= n, ldu >= n, leading dimensions that are multiples of
 * 16 bytes and 16-byte aligned l_dev, workspace_dev and u_dev. */
int cimrgp_trtri_rows(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, int64_t r0,
                      int64_t m, void* u_dev, int64_t ldu, void* stream);

/* Bytes of scratch cimrgp_kinv_diag needs to work in strips of strip_rows rows (rounded up to a multiple of 256, at
 * least 256, at most n rounded up to 256): strip x ldu x element size, ldu = n rounded up to 16 elements.  0 for an
 * unknown dtype or n < 1.  The batched call needs batch times as much. */
size_t cimrgp_kinv_diag_scratch_bytes(int dtype, int64_t n, int64_t strip_rows);

/* diag_out[i] = [K^-1]_ii = |row i of L^-T|^2, i in [0, n): cimrgp_trtri_rows strip by strip through scratch_dev,
 * each strip reduced by a row-sum-of-squares kernel (a workgroup per row, from the row's own panel on, fixed order).
 * The strip is as high as scratch_bytes allows (a multiple of 256; at least cimrgp_kinv_diag_scratch_bytes(dtype, n,
 * 256) is required); the result does not depend on it, bit for bit.  scratch_dev 16-byte aligned. */
int cimrgp_kinv_diag(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* scratch_dev,
                     size_t scratch_bytes, void* diag_out_dev, void* stream);

/* The same for `batch` equal-sized factors in the same launches (grid.y = block): factor b at l_dev + b * l_stride
 * (elements), its workspace at workspace_dev + b * workspace_stride_bytes (as in cimrgp_trsm_rows_lt_batched); diag_out
 * is (batch x n).  The scratch is shared evenly: every block gets a strip of the same height, and scratch_bytes must be
 * at least batch * cimrgp_kinv_diag_scratch_bytes(dtype, n, 256). */
int cimrgp_kinv_diag_batched(int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride,
                             const void* workspace_dev, size_t workspace_stride_bytes, void* scratch_dev,
                             size_t scratch_bytes, void* diag_out_dev, int batch, void* stream);

/* The O(n q) tail:  mean_out[i][c] = y[i][c] - alpha[i][c] / diag[i]  (n x q),  var_out[i] = 1 / diag[i]  (n).
 * q in [1, 8]; either output may be NULL (both: nothing is done). */
int cimrgp_loo(int dtype, const void* y_dev, const void* alpha_dev, const void* diag_dev, int64_t n, int q,
               void* mean_out_dev, void* var_out_dev, void* stream);

/* The same for the blocks of a layer: block b's targets are rows starts_dev[b] .. + n of y_dev, and so are its rows of
 * mean_out_dev (N x q) and var_out_dev (N); alpha_dev is (batch x n x q), diag_dev (batch x n). */
int cimrgp_loo_batched(int dtype, const void* y_dev, const int64_t* starts_dev, const void* alpha_dev,
                       const void* diag_dev, int64_t n, int q, int batch, void* mean_out_dev, void* var_out_dev,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_LOO_H */
