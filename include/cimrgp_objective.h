/* cimrgp_objective.h -- the hyper-parameter objective of the dense multiresolution model's layers.
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, CIMRGP_COV_*, CIMRGP_INFO_WATCHDOG, the
 * 0 / <0 return convention and cimrgp_last_error are defined there).  Kept in a header of its own: the entry points
 * of cimrgp.h are the model's fit and prediction path; these two serve the optional per-layer hyper-parameter
 * search (MultiResolutionGaussianProcess(optimize_hyperparameters=True)). */
#ifndef CIMRGP_OBJECTIVE_H
#define CIMRGP_OBJECTIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Log marginal likelihood and its gradient for `batch` equal-sized blocks of one layer (the objective of the
 * per-layer hyper-parameter search), with the addressing of cimrgp_layer_fit_cov: block b is rows
 * starts_dev[b] .. + n of x / y / fbar (fbar may be NULL).  For each block
 *   r_b = y - fbar - bias_b   (bias_b = *shared_bias_dev (q) if given, else the block's column means),
 *   K_b = k_cov(x_b, x_b) + noise I,  alpha = K_b^-1 r_b,
 *   out_dev[4b + 0] = LML_b = -1/2 sum_c r_c^T K_b^-1 r_c - q sum_i log L_ii - 1/2 n q log 2 pi,
 *   out_dev[4b + 1 .. 3] = d LML_b / d (log sf2, log ell, log noise) = 1/2 tr((alpha alpha^T - q K_b^-1) dK_b/dtheta),
 * doubles.  k_arena_dev (batch blocks of n x ldk, k_stride apart) receives L_b, kinv_arena_dev (same layout) the lower
 * triangle of K_b^-1 (the strict upper triangle of each n x n block holds junk; the columns [n, ldk) and the gaps
 * between the blocks of either arena are not written); ws_arena_dev as for cimrgp_layer_fit; info_dev[b] as for cimrgp_potrf (CIMRGP_INFO_WATCHDOG
 * included): a block with info != 0 has undefined outputs, the other blocks' outputs are not affected.
 * scratch_dev: cimrgp_layer_lml_grad_scratch_bytes(dtype, n, q, batch) bytes, 16-byte aligned (0 for invalid sizes).
 * Enqueue-only.  Every argument is checked before any device work (errors name cimrgp_layer_lml_grad_cov). */
size_t cimrgp_layer_lml_grad_scratch_bytes(int dtype, int64_t n, int q, int batch);
int cimrgp_layer_lml_grad_cov(int dtype, int cov, const void* x_dev, const void* y_dev,
                              const void* fbar_dev, const int64_t* starts_dev, int batch,
                              int64_t n, int d, int q, double ell, double sf2, double noise,
                              const void* shared_bias_dev,
                              void* k_arena_dev, int64_t ldk, int64_t k_stride,
                              void* kinv_arena_dev,
                              void* ws_arena_dev, size_t ws_stride_bytes, int32_t* info_dev,
                              void* scratch_dev, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_OBJECTIVE_H */
