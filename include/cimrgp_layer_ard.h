/* cimrgp_layer_ard.h -- the hyper-parameter objective of the multiresolution model's layers with one length-scale per
 * input dimension (ARD; DESIGN.md, "ARD length-scales for the model's layers").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, CIMRGP_COV_*, CIMRGP_INFO_WATCHDOG, the 0 / <0 return
 * convention and cimrgp_last_error are defined there).  The twin of cimrgp_layer_lml_grad_cov (cimrgp_objective.h) under
 * the convention of cimrgp_cov_lml_grad_ard: the caller divides its inputs by the length-scales, the covariance runs at
 * unit length-scale, and the gradient w.r.t. log l_k is 1/2 sum_ij G_ij (dk / dlog l_k)(xs_i, xs_j) per dimension. */
#ifndef CIMRGP_LAYER_ARD_H
#define CIMRGP_LAYER_ARD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch cimrgp_layer_lml_grad_ard_cov needs: cimrgp_layer_lml_grad_scratch_bytes' layout with tile records of
 * 10 doubles (sf | l_1 .. l_8 | trace) instead of 3, so never less than that.  0 for invalid sizes. */
size_t cimrgp_layer_lml_grad_ard_scratch_bytes(int dtype, int64_t n, int q, int batch);

/* Log marginal likelihood and its gradient for `batch` equal-sized blocks of one layer under an ARD covariance.
 * Everything is cimrgp_layer_lml_grad_cov's but for:
 *   xs_dev holds the inputs already divided by their length-scales (block b: rows starts_dev[b] .. + n of xs / y / fbar),
 *   K_b = k_cov(xs_b, xs_b) at unit length-scale + noise I,
 *   the record of block b has d + 3 doubles:
 *     out_dev[(d + 3) b + 0]           = LML_b
 *     out_dev[(d + 3) b + 1]           = d LML_b / d log sf2
 *     out_dev[(d + 3) b + 2 + k]       = d LML_b / d log l_k,  k = 0 .. d - 1
 *     out_dev[(d + 3) b + d + 2]       = d LML_b / d log noise.
 * dk / dlog l_k of the Matern 1/2 covariance at r = 0 is taken as 0, as in cimrgp_cov_lml_grad_ard.
 * Arenas, ws_arena_dev, info_dev (a block with info != 0 has undefined outputs, the other blocks' outputs are not
 * affected) and the alignment rules are the twin's.  scratch_dev: cimrgp_layer_lml_grad_ard_scratch_bytes(dtype, n, q,
 * batch) bytes, 16-byte aligned.  Enqueue-only.  Every argument is checked before any device work (errors name
 * cimrgp_layer_lml_grad_ard_cov). */
int cimrgp_layer_lml_grad_ard_cov(int dtype, int cov, const void* xs_dev, const void* y_dev,
                                  const void* fbar_dev, const int64_t* starts_dev, int batch,
                                  int64_t n, int d, int q, double sf2, double noise,
                                  const void* shared_bias_dev,
                                  void* k_arena_dev, int64_t ldk, int64_t k_stride,
                                  void* kinv_arena_dev,
                                  void* ws_arena_dev, size_t ws_stride_bytes, int32_t* info_dev,
                                  void* scratch_dev, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_LAYER_ARD_H */
