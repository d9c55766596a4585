/* cimrgp_sparse_layer.h -- the two device calls a sparse (inducing-point) LAYER of the multiresolution model adds to
 * include/cimrgp_sparse.h ("Sparse layers in the multiresolution model").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h.  A block of a layer takes its noise variance and its bias
 * from device scalars (cimrgp_noise_from_stats, cimrgp_block_stats): with the host-scalar calls of cimrgp_sparse.h the
 * fit would have to read them back.  Each call below is the twin of one of those over the same kernel body: notation,
 * memory footprint, argument rules and the 0 / <0 return convention are the twin's, and with the same values the results
 * are the twin's bit for bit.  Enqueue-only; every argument is checked before any device work (errors name the entry
 * point called). */
#ifndef CIMRGP_SPARSE_LAYER_H
#define CIMRGP_SPARSE_LAYER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cimrgp_sparse_lambda with the noise variance read from the device: noise_dev points to ONE element of dtype (not
 * NULL), read by the kernel when it runs.  Everything else as cimrgp_sparse_lambda. */
int cimrgp_sparse_lambda_dev(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, double sf2, const void* noise_dev,
                             int mode, void* lam_dev, void* w_dev, double* sums_dev, void* stream);

/* cimrgp_sparse_tail with two more device inputs, either of which may be NULL:
 *   bias_dev (q elements of dtype):       mean[i][c] (+)= (sum_j W*[i][j] gamma[j][c]) + bias[c]
 *   extra_var_dev (one element of dtype): var[i]     (+)= sf2 + extra_var + extra_var_dev[0] - sum A*^2 + sum W*^2
 * Both are added in FP64 behind the sums; the result is rounded to dtype once.  With both NULL the call is
 * cimrgp_sparse_tail.  bias_dev is read only with mean_dev, extra_var_dev only with var_dev.  (With W* = A, gamma = b
 * and bias_dev this is also the training-point prediction A b + bias of a fitted block.) */
int cimrgp_sparse_tail_dev(int dtype, const void* astar_dev, const void* wstar_dev, int64_t ns, int64_t m, int64_t lda,
                           const void* gamma_dev, int q, double sf2, double extra_var, const void* bias_dev,
                           const void* extra_var_dev, void* mean_dev, void* var_dev, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_LAYER_H */
