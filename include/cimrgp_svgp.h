/* cimrgp_svgp.h -- the non-conjugate part of the variational sparse GP ("Variational sparse GP with a
 * Student-t likelihood"): the expectation of a log-likelihood under q(f_i) = N(m_i, v_i) by Gauss-Hermite quadrature,
 * with its derivatives, fused into the row pass over A and W.
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, the 0 / <0 return convention and cimrgp_last_error are
 * defined there).  Notation of cimrgp_sparse.h, whitened: K_uu + (jitter sf + white) I = L_u L_u^T, A = K(X, Z) L_u^-T,
 * and per output column q(v) = N(mu, (P P^T)^-1) with P lower triangular: W = A P^-T, gamma = P^T mu,
 *   m_i = sum_j W_ij gamma_j,     v_i = kdiag_i - sum_j A_ij^2 + sum_j W_ij^2.
 * Every call is enqueue-only (no host read-back) and checks all of its arguments before any device work (errors name
 * the entry point). */
#ifndef CIMRGP_SVGP_H
#define CIMRGP_SVGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Likelihood ids of cimrgp_svgp_rows: log p(y | f) with e = y - f,
 *   GAUSSIAN   -1/2 log(2 pi s2) - e^2 / (2 s2)
 *   STUDENT_T  lgamma((nu + 1) / 2) - lgamma(nu / 2) - 1/2 log(nu pi s2) - (nu + 1) / 2 log1p(e^2 / (nu s2)). */
#define CIMRGP_LIK_GAUSSIAN 0
#define CIMRGP_LIK_STUDENT_T 1

/* Most quadrature nodes cimrgp_svgp_rows takes: one per lane of a wave. */
#define CIMRGP_SVGP_MAX_NODES 64

/* Rows per workgroup of the first stage of cimrgp_svgp_rows' sums over the rows; it sizes the scratch. */
#define CIMRGP_SVGP_SUM_CHUNK 2048

/* One pass over A and W (n x m, row-major, common pitch ld) for ONE output column, with gamma (m), kdiag (n), the targets
 * y_i = y_dev[i * y_stride] (column c of an n x q array is read in place: y_dev = its element c, y_stride = q) and the
 * H Gauss-Hermite nodes x_h and weights omega_h in nodes_dev (2 H doubles: the nodes, then the weights):
 *   E_i  = pi^-1/2 sum_h omega_h log p(y_i | f_ih),        f_ih = m_i + sqrt(2 v_i) x_h
 *   g1_i = dE_i / dm_i = pi^-1/2 sum_h omega_h l'(f_ih)                        l' = d log p / d f
 *   g2_i = dE_i / dv_i = pi^-1/2 sum_h omega_h l'(f_ih) x_h / sqrt(2 v_i)
 *   sums = [sum_i E_i, sum_i dE_i / dlog s2, #(v_i <= 0 or NaN)]               (3 doubles)
 * g1, g2 and the second sum are the exact derivatives of the quadrature sum.  A row with v_i <= 0 or NaN is counted,
 * adds nothing to the other two sums and has g1_i = g2_i = 0; its m_i and v_i are written as they are.
 * mean_dev, var_dev, g1_dev, g2_dev (n elements of the dtype each) and sums_dev may each be NULL; with sums_dev,
 * scratch_dev holds 3 (n + ceil(n / CIMRGP_SVGP_SUM_CHUNK)) doubles (the rows' terms, then the partial sums of chunks of
 * rows, which two more kernels add), else it may be NULL.
 * A wave per row: lane l adds columns l, l + 64, .. in FP64, the 64 partial sums are added pairwise, then the nodes are
 * evaluated one per lane in FP64 and added in the same order: a row's results depend on its own data and m alone, not
 * on n or on where the row lies.  The three sums are FP64 in a fixed order that depends on n alone.  No atomics: every
 * output is bit-identical from run to run.  Columns >= m and rows >= n of A and W are never read.
 * Requires 1 <= n < 2^31, 1 <= m < 2^31, ld >= m, y_stride >= 1, 1 <= nodes <= CIMRGP_SVGP_MAX_NODES, s2 > 0, and
 * nu > 0 for the Student-t (the Gaussian ignores it). */
int cimrgp_svgp_rows(int dtype, const void* a_dev, const void* w_dev, int64_t n, int64_t m, int64_t ld,
                     const void* gamma_dev, const void* kdiag_dev, const void* y_dev, int64_t y_stride,
                     const double* nodes_dev, int nodes, int likelihood, double s2, double nu, void* mean_dev,
                     void* var_dev, void* g1_dev, void* g2_dev, double* sums_dev, double* scratch_dev, void* stream);

/* Bytes of scratch cimrgp_svgp_moments needs: cimrgp_wsyrk_tn_scratch_bytes(dtype, n, m, q) (cimrgp_sparse.h). */
size_t cimrgp_svgp_moments_scratch_bytes(int dtype, int64_t n, int64_t m, int q);

/* The two m-sized moments of the row results in ONE pass over A (n x m, row-major, pitch lda):
 *   lower(C) = A^T diag(w) A   (m x m, pitch ldc; the strict upper triangle is not written)        N, with w = g2
 *   g        = A^T r           (m x q, row-major; r is n x q and is NOT weighted by w)             a, with r = g1
 * w may be of either sign and may hold zeros (the Student-t is not log-concave), which is why g cannot be had from
 * cimrgp_wsyrk_tn's weighted g by a division.  The kernels, the slicing of the rows and the fixed-order second kernel are
 * cimrgp_wsyrk_tn's: bit-identical from run to run, C equal to cimrgp_wsyrk_tn's with the same w and diag_add = 0 bit for
 * bit, and with r_dev = NULL (g_dev is then not written, q is ignored) the call IS that call.  Requirements as
 * cimrgp_wsyrk_tn's, with scratch_bytes >= cimrgp_svgp_moments_scratch_bytes(dtype, n, m, q). */
int cimrgp_svgp_moments(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* w_dev,
                        const void* r_dev, int q, void* c_dev, int64_t ldc, void* g_dev, void* scratch_dev,
                        size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SVGP_H */
