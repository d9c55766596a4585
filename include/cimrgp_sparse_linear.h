/* cimrgp_sparse_linear.h -- the sparse (inducing-point) GP with a linear term added to its covariance ("A linear
 * term for the sparse GP"):
 *   k(x, x') = k_cov(x, x') + sum_e lin_e x_e x'_e,
 * k_cov one of the CIMRGP_COV_* covariances and lin_e >= 0 one weight per input dimension (GPy's Linear(d, ARD=True)).
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h (dtype, covariance ids, the 0 / <0 return convention and
 * cimrgp_last_error are defined there).  k(x, x) is no longer the constant sf2, which three calls of the sparse path have
 * in their signatures; their twins are here.  In every call lin_dev is `const double*`: d FP64 values on the device, for
 * both dtypes; NULL is refused (the twins without the term exist for that).  Every call is enqueue-only and checks all of
 * its arguments before any device work. */
#ifndef CIMRGP_SPARSE_LINEAR_H
#define CIMRGP_SPARSE_LINEAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cimrgp_cov_gram with the linear term: K_ij = k_cov(x_i, x_j) + sum_e lin[e] x_ie x_je (+ diag_add on the diagonal).
 * Everything else is cimrgp_cov_gram's (cimrgp.h), with one exception: the lower triangle (lower_only != 0) is always
 * written in 64 x 64 tiles.  The lane rounds lin[e] x_je to the dtype once and an element costs d more multiply-adds in
 * the dtype, added to k_cov before diag_add.  With lin = 0 the output is cimrgp_cov_gram's 64 x 64-tile output bit for bit. */
int cimrgp_cov_gram_lin(int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2,
                        const double* lin_dev, double diag_add, void* k_dev, int64_t ldk, int lower_only, void* stream);

/* cimrgp_cov_cross with the linear term: K_ij = k_cov(xa_i, xb_j) + sum_e lin[e] xa_ie xb_je.  With lin = 0 the output is
 * cimrgp_cov_cross's bit for bit. */
int cimrgp_cov_cross_lin(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d,
                         double ell, double sf2, const double* lin_dev, void* kab_dev, int64_t ld, void* stream);

/* cimrgp_sparse_lambda (cimrgp_sparse.h) with k(x_i, x_i) read per row from kdiag_dev (n elements of the dtype) in place
 * of the constant sf2: q_i = sum_j A_ij^2,
 *   lam[i] = kdiag[i] - q_i + noise (mode 0, FITC) | noise (mode 1, VFE),   w[i] = 1 / lam[i],
 *   sums = [sum log lam_i, sum (kdiag[i] - q_i), #(lam_i <= 0)].
 * The same kernels and summation orders as the twin: with kdiag[i] = sf2 for every i (sf2 a value of the dtype) the three
 * outputs are the twin's bit for bit. */
int cimrgp_sparse_lambda_kd(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* kdiag_dev,
                            double noise, int mode, void* lam_dev, void* w_dev, double* sums_dev, void* stream);

/* Bytes of scratch cimrgp_cov_pair_grad_lin needs: those of cimrgp_cov_pair_grad (ard == 0) or cimrgp_cov_pair_grad_ard
 * (ard != 0) plus a second array of the partial db's size (128 d doubles per slice and column tile) for the partial P.
 * 0 for sizes outside [1, CIMRGP_PAIR_GRAD_MAX_NA] x [1, CIMRGP_PAIR_GRAD_MAX_NB] x [1, 8]. */
size_t cimrgp_cov_pair_grad_lin_scratch_bytes(int64_t na, int64_t nb, int d, int ard);

/* The pair contraction of the sparse objective's gradient under k = k_cov + linear: cimrgp_cov_pair_grad (ard == 0, sums_dev
 * 2 doubles; cimrgp_sparse_grad.h) or cimrgp_cov_pair_grad_ard (ard != 0, sums_dev 1 + d doubles; cimrgp_sparse_ard.h)
 * with, for P = G^T xa (nb x d),
 *   sums[...]   unchanged: the covariance part only, the twin's bits
 *   lsums[e]    (+)= sum_j xb_je P_je = sum_ij G_ij xa_ie xb_je                       e = 0 .. d - 1
 *   db[j][e]    (+)= scale (the twin's sum + lin[e] P_je)
 * lsums_e is the derivative of sum_ij G_ij k(xa_i, xb_j) w.r.t. lin_e; it is not scaled.  P is accumulated in FP64 from the
 * same single read of G (G is never read twice); its partials go to scratch beside the partial db, and the second kernel
 * adds them in slice order, then folds them into db and, over j in a fixed order, into lsums.  No atomics: bit-identical
 * from run to run.  With lin = 0, db is the twin's bit for bit.
 * sums_dev, lsums_dev (d doubles) and db_dev may each be NULL (all three: nothing is done); accumulate != 0 adds to what
 * the given outputs hold.  Requirements as the twin's, with scratch_bytes >= cimrgp_cov_pair_grad_lin_scratch_bytes(na,
 * nb, d, ard). */
int cimrgp_cov_pair_grad_lin(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d,
                             const void* g_dev, int64_t ldg, double ell, double sf2, int ard, const double* lin_dev,
                             double scale, int accumulate, double* sums_dev, double* lsums_dev, void* db_dev,
                             void* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_SPARSE_LINEAR_H */
