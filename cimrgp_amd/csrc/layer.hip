// One C call per layer for a batch of equal-sized blocks (round 3): the reference's independent-over-l
// loops -- fit: Posteriors.py:35-59 (update_scale_given_axis over the regions of a resolution),
// predict: MRGP.py:782-803 (per-region predictions of a resolution, concatenated) -- with every step
// launched ONCE for all the blocks (blockIdx.y = block).  Regions are contiguous ranges of the layer's
// arrays (Inputs.py:57-60), so a block is a row offset (`starts`) into x / y / f_bar.
//
//   fit      statistics -> bias, noise | residual rows | Gram + noise | factorisation with the residual
//            rows carried (z = L^-1 r) | backward solve (alpha) | training-point prediction
//   predict  cross-Gram | row-wise solve W = K* L^-T | mean = W z + bias, var = sf - sum W^2 (+ noise)
// Two steps are shared: fit_front_run (everything of the fit up to alpha; also the front end of the log marginal
// likelihood, with the identity among the carried rows) and cross_solve_run (predict's first two steps; also the W of the
// joint covariance, joint.hip, and of the predictive gradient, grad.hip).
// The Gram and cross-Gram take the layer's covariance policy (a.cov, CIMRGP_COV_*); k(0) = sf for every policy, so
// the variance is the same expression for all of them.
//
// Round 2 issued five launches per block from a Python loop for the front end and one row-wise solve
// per block for the prediction: a layer of 128 blocks of 2048 points was launch-bound (22 ms for 0.37
// Tflop).
#include "common.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

// Per block b: column means of (y - f_bar) and the pooled population variance about them
// (block_stats, reduce.hpp: the body of k_block_stats, misc.hip), then
//   bias[b]  = the shared bias if given, else the column means
//   noise[b] = the fixed value if >= 0, else the shared noise if given, else max(frac var, floor)
// (RegressionInput.py:62: labels.var() * 0.01).
template <typename T>
__global__ __launch_bounds__(1024)
void k_layer_stats(const T* __restrict__ y, const T* __restrict__ fbar, const int64_t* __restrict__ starts, int64_t n, int q,
                   T noise_fixed, T frac, T floor_value, const T* __restrict__ shared_bias,
                   const T* __restrict__ shared_noise, T* __restrict__ bias, T* __restrict__ noise)
{
    __shared__ T red[16];
    __shared__ T smean[MAXQ];
    const int b = blockIdx.x;
    const T* yb = y + starts[b] * q;
    const T* fb = fbar ? fbar + starts[b] * q : nullptr;
    const T var = block_stats(yb, fb, n, q, red, smean);
    if (threadIdx.x == 0) {
        for (int c = 0; c < q; ++c) bias[(int64_t)b * q + c] = shared_bias ? shared_bias[c] : smean[c];
        T v;
        if (noise_fixed >= (T)0) v = noise_fixed;
        else if (shared_noise) v = shared_noise[0];
        else {
            v = frac * var;
            if (!(v > floor_value)) v = floor_value;
        }
        noise[b] = v;
    }
}

// rows[b][c][j] = y - f_bar - bias: the block's residual, transposed, as the q rows carried through the
// factorisation
template <typename T>
__global__ void k_layer_rows(const T* __restrict__ y, const T* __restrict__ fbar, const int64_t* __restrict__ starts,
                             int64_t n, int q, const T* __restrict__ bias, T* __restrict__ rows, int64_t ldr, int64_t srows)
{
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * q) return;
    const int64_t j = e / q;
    const int c = (int)(e - j * q);
    const int64_t g = (starts[b] + j) * q + c;
    rows[(int64_t)b * srows + (int64_t)c * ldr + j] = y[g] - (fbar ? fbar[g] : (T)0) - bias[(int64_t)b * q + c];
}

// z[b][j][c] = alpha0[b][j][c] = rows[b][c][j] (z = L^-1 r after the factorisation; alpha0 is solved in place)
template <typename T>
__global__ void k_layer_z(const T* __restrict__ rows, int64_t ldr, int64_t srows, int64_t n, int q, T* __restrict__ z,
                          T* __restrict__ alpha, T* __restrict__ work, int64_t swork)
{
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * q) return;
    const int64_t j = e / q;
    const int c = (int)(e - j * q);
    const T v = rows[(int64_t)b * srows + (int64_t)c * ldr + j];
    z[(int64_t)b * n * q + e] = v;
    alpha[(int64_t)b * n * q + e] = v;
    // the backward solve's running right-hand side (q x n per problem, potrs_run: `work`), so that it need not transpose alpha first
    if (work) work[(int64_t)b * swork + (int64_t)c * n + j] = v;
}

// train_out += K_noiseless alpha + bias = (y - f_bar - bias) - noise alpha + bias = y - f_bar - noise alpha
// (no second pass over the Gram matrix: K alpha = r - noise alpha)
template <typename T>
__global__ void k_layer_train_mean(const T* __restrict__ y, const T* __restrict__ fbar, const int64_t* __restrict__ starts,
                                   int64_t n, int q, const T* __restrict__ alpha, const T* __restrict__ noise,
                                   T* __restrict__ out)
{
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * q) return;
    const int64_t g = starts[b] * q + e;
    out[g] += y[g] - (fbar ? fbar[g] : (T)0) - noise[b] * alpha[(int64_t)b * n * q + e];
}

}  // namespace

// rows[b][q + i][j] = (i == j): the identity below the q residual rows
template <typename T>
__global__ void k_layer_eye(T* __restrict__ rows, int64_t ldr, int64_t srows, int64_t n, int q)
{
    const int64_t b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int64_t i = e / n, j = e - i * n;
    rows[b * srows + (q + i) * ldr + j] = (i == j) ? (T)1 : (T)0;
}

// The fit up to alpha, in the name of the entry point fn: bias, noise | carried rows (the residual, then the identity if
// a.eye) | Gram + noise | factorisation with the rows carried | z, alpha0, work | backward solve
template <typename T>
static int fit_front_run(const FitFront<T>& a, hipStream_t st, const char* fn)
{
    const int64_t n = a.tr.n;
    const unsigned nb = (unsigned)a.bc.batch;
    const unsigned ge = (unsigned)((n * a.q + 255) / 256);
    hipLaunchKernelGGL((k_layer_stats<T>), dim3(nb), dim3(1024), 0, st, a.y, a.fbar, a.tr.starts, n, a.q, (T)a.noise_fixed,
                       (T)a.noise_frac, (T)a.noise_floor, a.shared_bias, a.shared_noise, a.bias, a.noise);
    CIMRGP_LAUNCH_CHECK(fn);
    hipLaunchKernelGGL((k_layer_rows<T>), dim3(ge, nb), dim3(256), 0, st, a.y, a.fbar, a.tr.starts, n, a.q, (const T*)a.bias,
                       a.rows.p, a.rows.ld, a.rows.stride);
    CIMRGP_LAUNCH_CHECK(fn);
    if (a.eye) {
        hipLaunchKernelGGL((k_layer_eye<T>), dim3((unsigned)((n * n + 255) / 256), nb), dim3(256), 0, st, a.rows.p, a.rows.ld,
                           a.rows.stride, n, a.q);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    int rc = rbf_gram_batched_run<T>(a.bc, a.tr, a.tr, (const T*)a.noise, a.f.l, true, st);
    if (rc) return rc;
    const PotrfBatch bt = potrf_batch(a.bc.batch, a.f, a.rows.stride);
    rc = potrf_batched_run<T>(a.f.l.p, n, a.f.l.ld, a.f.ws, a.info, a.rows.p, a.q + (a.eye ? n : 0), a.rows.ld, bt, st);
    if (rc) return rc;
    hipLaunchKernelGGL((k_layer_z<T>), dim3(ge, nb), dim3(256), 0, st, (const T*)a.rows.p, a.rows.ld, a.rows.stride, n, a.q, a.z,
                       a.alpha, a.work, 2 * (int64_t)a.q * n);
    CIMRGP_LAUNCH_CHECK(fn);
    return potrs_run<T>(a.f.l.p, n, a.f.l.ld, a.f.ws, a.alpha, a.q, nullptr, a.work, true, st, bt, true);
}

template <typename T>
int layer_fit_run(const LayerFit<T>& a, hipStream_t st)
{
    const char* fn = "cimrgp_layer_fit";
    const FitFront<T>& fr = a.fr;
    CIMRGP_REQUIRE(fr.bc.batch >= 1 && fr.bc.batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(fr.tr.n > 0, fn, "empty blocks");
    CIMRGP_REQUIRE(fr.q >= 1 && fr.q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    const int rc = fit_front_run<T>(fr, st, fn);
    if (rc) return rc;
    hipLaunchKernelGGL((k_layer_train_mean<T>), dim3((unsigned)((fr.tr.n * fr.q + 255) / 256), (unsigned)fr.bc.batch), dim3(256), 0, st,
                       fr.y, fr.fbar, fr.tr.starts, fr.tr.n, fr.q, (const T*)fr.alpha, (const T*)fr.noise, a.train_out);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int cross_solve_run(const BatchCov& bc, const Points<T>& train, const Factors<const T>& f, const Points<T>& tests, const Arena<T>& w,
                    hipStream_t st)
{
    // W_b = K(xs_b, x_b)
    const int rc = rbf_gram_batched_run<T>(bc, tests, train, (const T*)nullptr, w, false, st);
    if (rc) return rc;
    // W_b <- W_b L_b^-T
    return solve_rows_run<T>(f.l.p, train.n, f.l.ld, f.ws, w.p, tests.n, w.ld, st, potrf_batch(bc.batch, f, w.stride));
}

template <typename T>
int layer_predict_run(const LayerPredict<T>& a, hipStream_t st)
{
    const char* fn = "cimrgp_layer_predict";
    CIMRGP_REQUIRE(a.bc.batch >= 1 && a.bc.batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(a.q >= 1 && a.q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    if (a.te.n <= 0 || a.tr.n <= 0) return 0;
    CIMRGP_REQUIRE(a.w.ld >= a.tr.n, fn, "leading dimension of W smaller than n");
    const int rc = cross_solve_run<T>(a.bc, a.tr, a.f, a.te, a.w, st);
    if (rc) return rc;
    // mean += W z + bias, var += sf - sum W^2 (+ noise)
    return predict_from_w_run<T>((const T*)a.w.p, a.te.n, a.tr.n, a.w.ld, a.z, a.q, a.bc.sf2, 0.0, a.noise, a.bias, a.mean, a.var, 1,
                                 st, a.bc.batch, a.te.starts, a.w.stride);
}

// ---- log marginal likelihood and its gradient for a batch of blocks (cimrgp_layer_lml_grad_cov, ..._ard_cov) ----
//   statistics -> bias | residual rows r^T and the identity as q + n carried rows | Gram + noise | factorisation with
//   the rows carried: z^T = r^T L^-T and U = L^-T come out of the same panel sweep | backward solve (alpha) |
//   lower(K^-1) = U U^T (batched SYRK on the matrix cores) | gradient tiles + per-block finish (misc.hip)
// K^-1 method: the identity rides through potrf_rows_batched as carried rows, then one batched SYRK: about
// n^3 + n^3 flops per block on top of the factorisation, all in kernels the factorisation already uses.

// k_b[0:n, 0:n] = 0 (the SYRK's C): the padding columns [n, ld) and the gaps between the blocks belong to the caller
template <typename T>
__global__ void k_layer_zero(T* __restrict__ k, int64_t ld, int64_t ks, int64_t n)
{
    const int64_t b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int64_t i = e / n, j = e - i * n;
    k[b * ks + i * ld + j] = (T)0;
}

// lower(k_b) = -lower(k_b): the SYRK subtracts (C -= A A^T)
template <typename T>
__global__ void k_layer_neg_lower(T* __restrict__ k, int64_t ld, int64_t ks, int64_t n)
{
    const int64_t b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int64_t i = e / n, j = e - i * n;
    if (j <= i) k[b * ks + i * ld + j] = -k[b * ks + i * ld + j];
}

LmlScratch lml_scratch_layout(size_t esz, int64_t n, int q, int batch, int np)
{
    LmlScratch s;
    s.ldr = padded_ld(n);                    // device.padded_ld's rule
    s.srows = (int64_t)(q + n) * s.ldr;
    auto seg = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    const size_t nb = (size_t)batch;
    size_t off = 0;
    s.rows = off;    off += seg(nb * (size_t)s.srows * esz);
    s.z = off;       off += seg(nb * (size_t)(n * q) * esz);
    s.alpha = off;   off += seg(nb * (size_t)(n * q) * esz);
    s.work = off;    off += seg(nb * (size_t)(2 * n * q) * esz);
    s.bias = off;    off += seg(nb * (size_t)q * esz);
    s.noise = off;   off += seg(nb * esz);
    s.partial = off; off += seg(nb * (size_t)lml_grad_tiles_count(n) * (size_t)np * sizeof(double));
    s.total = off;
    return s;
}

template <typename T>
int layer_lml_grad_run(const LayerLml<T>& a, hipStream_t st, bool ard)
{
    const char* fn = ard ? "cimrgp_layer_lml_grad_ard_cov" : "cimrgp_layer_lml_grad_cov";
    FitFront<T> fr = a.fr;
    const int64_t n = fr.tr.n;
    CIMRGP_REQUIRE(fr.bc.batch >= 1 && fr.bc.batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n > 0 && n < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(fr.q >= 1 && fr.q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    const LmlScratch sl = lml_scratch_layout(sizeof(T), n, fr.q, fr.bc.batch, lml_grad_record_width(ard));
    char* base = (char*)a.scratch;
    fr.rows = Arena<T>{(T*)(base + sl.rows), sl.ldr, sl.srows};
    fr.eye = true;
    fr.z = (T*)(base + sl.z);
    fr.alpha = (T*)(base + sl.alpha);
    fr.work = (T*)(base + sl.work);
    fr.bias = (T*)(base + sl.bias);
    fr.noise = (T*)(base + sl.noise);
    double* partial = (double*)(base + sl.partial);
    int rc = fit_front_run<T>(fr, st, fn);
    if (rc) return rc;
    const Arena<T>& k = fr.f.l;
    const dim3 grid((unsigned)((n * n + 255) / 256), (unsigned)fr.bc.batch);
    hipLaunchKernelGGL((k_layer_zero<T>), grid, dim3(256), 0, st, a.kinv, k.ld, k.stride, n);
    CIMRGP_LAUNCH_CHECK(fn);
    const T* u = fr.rows.p + (int64_t)fr.q * sl.ldr;
    rc = gemm_nt_sub<T>(a.kinv, k.ld, u, sl.ldr, u, sl.ldr, n, n, (int)n, true, st, gemm_batch(fr.bc.batch, k.stride, sl.srows, sl.srows));
    if (rc) return rc;
    hipLaunchKernelGGL((k_layer_neg_lower<T>), grid, dim3(256), 0, st, a.kinv, k.ld, k.stride, n);
    CIMRGP_LAUNCH_CHECK(fn);
    return lml_grad_batched_run<T>(fr.tr.x, fr.tr.starts, fr.bc.batch, n, fr.bc.d, (const T*)a.kinv, k.ld, k.stride, (const T*)k.p,
                                   (const T*)fr.alpha, (const T*)fr.z, fr.q, fr.bc.ell, fr.bc.sf2, fr.noise_fixed, a.out, partial, st,
                                   fr.bc.cov, fn, ard);
}

// The targets of ONE block as carried rows and back (cimrgp_block_posterior).
template <typename T>
__global__ void k_rhs_rows(const T* __restrict__ y, int64_t n, int q, T* __restrict__ rows, int64_t ldr)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * q) return;
    const int64_t j = e / q;
    const int c = (int)(e - j * q);
    rows[(int64_t)c * ldr + j] = y[e];
}

template <typename T>
int rhs_rows_run(const T* y, int64_t n, int q, T* rows, int64_t ldr, hipStream_t st)
{
    if (n <= 0 || q <= 0) return 0;
    hipLaunchKernelGGL((k_rhs_rows<T>), dim3((unsigned)((n * q + 255) / 256)), dim3(256), 0, st, y, n, q, rows, ldr);
    CIMRGP_LAUNCH_CHECK("cimrgp_block_posterior");
    return 0;
}

template <typename T>
int rows_to_z_run(const T* rows, int64_t ldr, int64_t n, int q, T* z, T* alpha, hipStream_t st, T* work)
{
    if (n <= 0 || q <= 0) return 0;
    hipLaunchKernelGGL((k_layer_z<T>), dim3((unsigned)((n * q + 255) / 256), 1), dim3(256), 0, st, rows, ldr, (int64_t)0, n, q, z, alpha,
                       work, (int64_t)0);
    CIMRGP_LAUNCH_CHECK("cimrgp_block_posterior");
    return 0;
}

template int rhs_rows_run<double>(const double*, int64_t, int, double*, int64_t, hipStream_t);
template int rhs_rows_run<float>(const float*, int64_t, int, float*, int64_t, hipStream_t);
template int rows_to_z_run<double>(const double*, int64_t, int64_t, int, double*, double*, hipStream_t, double*);
template int rows_to_z_run<float>(const float*, int64_t, int64_t, int, float*, float*, hipStream_t, float*);
template int layer_fit_run<double>(const LayerFit<double>&, hipStream_t);
template int layer_fit_run<float>(const LayerFit<float>&, hipStream_t);
template int cross_solve_run<double>(const BatchCov&, const Points<double>&, const Factors<const double>&, const Points<double>&,
                                     const Arena<double>&, hipStream_t);
template int cross_solve_run<float>(const BatchCov&, const Points<float>&, const Factors<const float>&, const Points<float>&,
                                    const Arena<float>&, hipStream_t);
template int layer_predict_run<double>(const LayerPredict<double>&, hipStream_t);
template int layer_predict_run<float>(const LayerPredict<float>&, hipStream_t);
template int layer_lml_grad_run<double>(const LayerLml<double>&, hipStream_t, bool);
template int layer_lml_grad_run<float>(const LayerLml<float>&, hipStream_t, bool);

}  // namespace cimrgp
