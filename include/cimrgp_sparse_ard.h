/* cimrgp_sparse_ard.h -- the pair contraction of the sparse (inducing-point) objective with one length-scale per input
 * dimension (ARD; DESIGN.md, "ARD length-scales for the sparse GP").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, covariance ids, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  The caller divides its inputs by the length-scales, so that the covariance runs
 * at one length-scale `ell` for all dimensions; what the gradient w.r.t. log l_e needs of the n x m weight matrix is then
 *   sum_ij G_ij (dk / dlog l_e)(xa_i, xb_j) = sum_ij G_ij g(r_ij) (xa_ie - xb_je)^2,
 * d sums from the same single read of G that cimrgp_cov_pair_grad (cimrgp_sparse_grad.h) makes for its one. */
#ifndef CIMRGP_SPARSE_ARD_H
#define CIMRGP_SPARSE_ARD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch cimrgp_cov_pair_grad_ard needs for an na x nb weight matrix and input dimension d: per slice and column
 * tile of 128 columns, 128 d partial sums of db and the 1 + d partial scalar sums, all FP64 (the same for both dtypes).
 * The slices are those of cimrgp_cov_pair_grad.  0 for sizes outside [1, CIMRGP_PAIR_GRAD_MAX_NA] x
 * [1, CIMRGP_PAIR_GRAD_MAX_NB] x [1, 8]. */
size_t cimrgp_cov_pair_grad_ard_scratch_bytes(int64_t na, int64_t nb, int d);

/* The twin of cimrgp_cov_pair_grad with the sum over dk/dlog l kept apart per input dimension: for G (na x nb, row-major,
 * pitch ldg), xa (na x d) and xb (nb x d), d in [1, 8],
 *   sums[0]     (+)= sum_ij G_ij k(xa_i, xb_j)
 *   sums[1 + e] (+)= sum_ij G_ij g(r_ij) (xa_ie - xb_je)^2                   e = 0 .. d - 1
 *   db[j][e]    (+)= scale sum_i G_ij g(r_ij) (xa_ie - xb_je)                (nb x d, row-major)
 * with g of cimrgp_grad.h (dk(a, b)/da_e = -g(r) (a_e - b_e); 0 at r = 0 for Matern 1/2).  g (a_e - b_e)^2 is dk/dlog l_e of
 * k(sqrt(sum_e ((a_e - b_e) / l_e)^2)) at l_e = ell for all e; summed over e it is cimrgp_cov_pair_grad's sums[1].
 * sums_dev (1 + d doubles) or db_dev may be NULL (both: nothing is done); accumulate != 0 adds to what both outputs
 * hold; scale multiplies the db sum only.  Everything else is cimrgp_cov_pair_grad's: k and g per pair in the dtype, the
 * products with G and all sums FP64; the same S slices; partial sums in scratch_dev added in slice (and tile) order by
 * a second kernel, no atomics, bit-identical from run to run; in FP64 sums[0] and db are bit-identical to
 * cimrgp_cov_pair_grad's.  G is read once; columns >= nb of G and rows >= na of G and xa are never read.
 * Requires 1 <= na <= CIMRGP_PAIR_GRAD_MAX_NA, 1 <= nb <= CIMRGP_PAIR_GRAD_MAX_NB, ldg >= nb, ell > 0, sf2 > 0,
 * scratch_dev 8-byte aligned, scratch_bytes >= cimrgp_cov_pair_grad_ard_scratch_bytes(na, nb, d). */
int cimrgp_cov_pair_grad_ard(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d,
                             const void* g_dev, int64_t ldg, double ell, double sf2, double scale, int accumulate,
                             double* sums_dev, void* db_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_ARD_H */
