/* cimrgp_psi_grad.h -- the derivatives of the psi statistics of cimrgp_psi.h, contracted with a weight matrix: what the
 * analytic gradient of the bound on uncertain inputs needs ("Gradients of the bound on uncertain inputs").
 *
 * Part of the C ABI of libcimrgp.so, included by cimrgp.h.  Notation, operands and conventions are those of
 * cimrgp_psi.h: x_i ~ N(mu_i, diag s_i), inducing inputs z_j, variance sf2, length-scales l_e (ell_dev, float64 on the
 * device); mu, s, dmu, ds are n x d, z and dz m x d, row-major without padding and of the call's dtype.  For a weight
 * matrix G the calls return the derivatives of F = sum G o Psi:
 *   dmu[i][e] = dF / dmu_ie      ds[i][e] = dF / ds_ie      dz[j][e] = dF / dz_je
 *   sums[0]   = dF / dlog sf2    (sum G o Psi1, 2 sum G o Psi2)
 *   sums[1+e] = dF / dlog l_e
 * sums is float64[d + 1] on the device.  Every output is OVERWRITTEN.  No atomics: every sum is taken in one fixed order
 * that depends on (n, m, d) alone, so two calls give the same bits.  There is no division by s: s_ie = 0 is exact.
 * Every call is enqueue-only on `stream` and checks all of its arguments before any device work.
 * Requires d in [1, 8], sf2 > 0, 1 <= n <= CIMRGP_PSI2_MAX_N, 1 <= m <= CIMRGP_PSI2_MAX_M, a 16-byte aligned scratch_dev
 * of at least the call's ..._scratch_bytes. */
#ifndef CIMRGP_PSI_GRAD_H
#define CIMRGP_PSI_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Workgroups the row passes aim at (the pair passes aim at CIMRGP_PSI2_TARGET_WGS, by the slice rule of cimrgp_psi.h). */
#define CIMRGP_PSI_GRAD_ROW_WGS 1024
/* Tile edge of the pairs pass of cimrgp_psi2_grad: a thread owns 4 x 4 pairs for d <= 2 and 2 x 2 beyond. */
#define CIMRGP_PSI_GRAD_PAIR_EDGE(d) ((d) <= 2 ? 64 : 32)

/* Bytes of scratch cimrgp_psi1_grad needs: with c = ceil(m / 64) column blocks and S slices of the rows by the slice
 * rule of cimrgp_psi.h for c workgroups per slice, S m d partial sums of dz (the dtype) and S c (d + 1) of sums
 * (float64), each part rounded up to 16 bytes.  0 for an unknown dtype or sizes outside the limits. */
size_t cimrgp_psi1_grad_scratch_bytes(int dtype, int64_t n, int64_t m, int d);

/* F = sum_ij g1[i][j] Psi1[i][j] for g1_dev (n x m, pitch ldg >= m).  Psi1 is recomputed as cimrgp_psi1 forms it, not
 * read.  With a = mu_ie - z_je and h = 1 / (l_e^2 + s_ie), each times g1_ij Psi1_ij:
 *   d/dmu_ie = -a h    d/dz_je = a h    d/ds_ie = 1/2 (a^2 h^2 - h)    d/dlog l_e = s h + l_e^2 a^2 h^2
 * Three kernels: a wave per row (dmu, ds: nothing is reduced across rows); a thread per column over one slice of the
 * rows, the rows' constants staged through LDS (partial dz and sums to scratch); the slices added in slice order. */
int cimrgp_psi1_grad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                     const double* ell_dev, double sf2, const void* g1_dev, int64_t ldg, void* dmu_dev, void* ds_dev,
                     void* dz_dev, double* sums_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* Bytes of scratch cimrgp_psi2_grad needs: one count per 256 rows (float64), the rows' 3 d + 1 constants, the P partial
 * dmu and ds of the rows pass (P n 2 d; P = max(1, min(tiles of 64 x 64 pairs, CIMRGP_PSI_GRAD_ROW_WGS / ceil(n / 256)))),
 * and per (slice, tile) of the pairs pass 2 E d partial sums of dz (E = CIMRGP_PSI_GRAD_PAIR_EDGE(d), tiles of E x E
 * pairs, slices by the slice rule for that tile count) and d + 1 of sums (float64); each part rounded up to 16 bytes.
 * 0 for an unknown dtype or sizes outside the limits. */
size_t cimrgp_psi2_grad_scratch_bytes(int dtype, int64_t n, int64_t m, int d);

/* F = sum_jk g2[j][k] Psi2[j][k] for a SYMMETRIC g2_dev (m x m, pitch ldg >= m) of which only k <= j is read: an
 * off-diagonal pair stands for both (j, k) and (k, j).  With term_ijk = sf2^2 exp(-delta_jk - t_ijk) (cimrgp_psi.h),
 * a = mu_ie - (z_je + z_ke) / 2 and r = 1 / (l_e^2 + 2 s_ie), each times g2_jk term_ijk:
 *   d/dmu_ie = -2 a r    d/ds_ie = 2 a^2 r^2 - r    d/dz_je = a r - (z_je - z_ke) / (2 l_e^2)
 *   d/dlog l_e = 2 s r + 2 l_e^2 a^2 r^2 + (z_je - z_ke)^2 / (2 l_e^2)
 * The exponent is taken in cimrgp_psi2's direct form.  Two passes pay the n m^2 / 2 exponentials each:
 *   rows   a thread per row walks the pairs of its share of the 64 x 64 tiles, z / 2 and the weights
 *          w g2_jk sf2^2 exp(-delta_jk) (w = 1 on the diagonal, 2 off it) staged in LDS; 2 d + 1 sums in registers
 *   pairs  cimrgp_psi2's geometry (one tile and one slice of the rows per workgroup, the rows' constants staged
 *          through LDS); a thread keeps the sums of its own points and pairs
 * and the partial sums are added in slice order.  A row with a negative or non-finite variance is counted in
 * bad_dev[0] (overwritten, as by cimrgp_psi2), adds nothing anywhere, and its rows of dmu and ds are zeros. */
int cimrgp_psi2_grad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                     const double* ell_dev, double sf2, const void* g2_dev, int64_t ldg, void* dmu_dev, void* ds_dev,
                     void* dz_dev, double* sums_dev, void* scratch_dev, size_t scratch_bytes, double* bad_dev,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIMRGP_PSI_GRAD_H */
