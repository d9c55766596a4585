/* cimrgp_joint.h -- the joint predictive distribution of the dense multiresolution model: block covariances, their
 * factors and posterior samples.
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, CIMRGP_COV_*, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  Layers are independent and, within a layer, the regions are conditionally
 * independent, so the joint covariance over a set of test points is a sum over the layers of block-diagonal matrices:
 * one ns_b x ns_b block per region, never N* x N* ("Joint predictive covariance and posterior samples").
 * All three calls take device pointers and a stream, are enqueue-only (no host read-back) and check every argument
 * before any device work (errors name the entry point). */
#ifndef CIMRGP_JOINT_H
#define CIMRGP_JOINT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Standard normals for `batch` blocks:  z_b[c * ldz + i] = phi(seed, keys_dev[b], col0 + c, i)  for c < cols, i < ns,
 * with z_b = z_dev + b * z_stride (elements of dtype).  Each sample column is a ROW of z_b (Z^T: the layout of
 * cimrgp_layer_sample).  keys_dev: batch uint64 values on the device.  Nothing but those cols x ns values per block is
 * written.  phi(seed, key, c, i), fixed here so that it can be restated anywhere (tests/test_joint_host.py in NumPy):
 *   x0..x3 = Philox4x32-10(counter = (i >> 1, c, key_lo, key_hi), key = (seed_lo, seed_hi))
 *            (Salmon et al. 2011: multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85)
 *   u1 = (((x1 << 32 | x0) >> 11) + 0.5) * 2^-53,  u2 the same from (x3 << 32 | x2)
 *   r  = sqrt(-2 ln u1);  phi = r cos(2 pi u2) for even i, r sin(2 pi u2) for odd i
 * evaluated in FP64 (FP32 output: the FP64 value rounded).  A value depends on (seed, key, c, i) only: not on the
 * batch, on the block's place in it, on ns or on cols, so a request for fewer columns gives a prefix of a longer one.
 * Requires cols >= 0, ns >= 0, col0 >= 0, col0 + cols <= 2^32, ldz >= ns and, for batch > 1,
 * z_stride >= (cols - 1) * ldz + ns. */
int cimrgp_normal_fill(int dtype, uint64_t seed, const uint64_t* keys_dev, int batch, int64_t col0, int64_t cols,
                       int64_t ns, void* z_dev, int64_t ldz, int64_t z_stride, void* stream);

/* Predictive covariance block of each of `batch` blocks of one layer, with the training side of
 * cimrgp_layer_predict_cov (x, starts, n, cov, ell, sf2, the factors L_b and their workspaces from cimrgp_layer_fit_cov)
 * and the block's ns test points at rows t_starts_dev[b] .. + ns of xs:
 *   W_b = K(xs_b, x_b) L_b^-T            (matrix b of w_arena_dev: ns x ldw, stride w_stride; a work area)
 *   lower(C_b) = K(xs_b, xs_b) + diag_dev[b] I - W_b W_b^T
 * in matrix b of c_arena_dev (ns x ldc, stride c_stride).  diag_dev: batch values of dtype (jitter, noise: the caller's
 * policy) or NULL for none.
 * cws_arena_dev == NULL: that is all; info_dev is not used.  The strict upper triangle of each ns x ns block may be
 * overwritten with junk (the Gram writes whole diagonal tiles, the update stores diagonal 128 x 128 tiles whole);
 * the columns [ns, ldc) and the gaps between the blocks are not written.
 * Otherwise each C_b is factored in place (L L^T, the workspace of cimrgp_potrf at byte stride cws_stride_bytes in
 * cws_arena_dev) and then the strict upper triangle of each ns x ns block is set to zero (only that block: the padding
 * and the gaps stay the caller's).  info_dev[b] follows the LAPACK convention (CIMRGP_INFO_WATCHDOG included); a block
 * with info != 0 has an undefined factor, the other blocks are not affected.  Requires n >= 1, ns >= 0 (0: nothing is
 * done), d in [1, 8], ell > 0, sf2 > 0, ldl >= n, ldw >= n (and at least 128 bytes), ldc >= ns, leading dimensions
 * and strides that are multiples of 16 bytes, 16-byte aligned arenas and, for batch > 1, strides that do not make
 * blocks overlap. */
int cimrgp_layer_joint_cov(int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d,
                           const void* xs_dev, const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2,
                           const void* l_arena_dev, int64_t ldl, int64_t l_stride, const void* ws_arena_dev,
                           size_t ws_stride_bytes, const void* diag_dev, void* w_arena_dev, int64_t ldw, int64_t w_stride,
                           void* c_arena_dev, int64_t ldc, int64_t c_stride, void* cws_arena_dev,
                           size_t cws_stride_bytes, int32_t* info_dev, void* stream);

/* Posterior sample paths of `batch` blocks:  out[c * ld_out + t_starts_dev[b] + i] += sum_{k <= i} L_b[i][k] z_b[c * ldz + k]
 * for c < cols, i < ns -- out^T += Z^T L^T per block (a new matrix-core kernel, k_layer_sample), with L_b = l_arena_dev +
 * b * l_stride (ns x ldl; only its lower triangle is read as such: whatever the strict upper triangle holds, NaN
 * included, does not reach out) and z_b = z_dev + b * z_stride (cols rows of ldz; the elements [ns, ldz) of a row may
 * be read, never used).  out is ONE (cols x ld_out) buffer shared by the blocks of a call (and across calls and
 * layers: the call accumulates); the blocks of one call must write disjoint test ranges (as for cimrgp_layer_predict).
 * Requires ldl >= ns, ldz >= ns, ld_out >= 1, ldl and ldz multiples of 16 bytes, at least 128 bytes and below 2^23
 * elements, 16-byte aligned l_arena_dev and z_dev. */
int cimrgp_layer_sample(int dtype, const void* l_arena_dev, int64_t ldl, int64_t l_stride, int64_t ns, int batch,
                        const void* z_dev, int64_t ldz, int64_t z_stride, int64_t cols, const int64_t* t_starts_dev,
                        void* out_dev, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_JOINT_H */
