// D6 / a11: small element-wise and reduction kernels of the residual chain.
// All HBM-bound and tiny (O(n q)); they exist so that the product path never
// leaves the device between blocks.
#include "common.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

// stats[c] = mean_i (y - fbar)[i][c];  stats[q] = pooled population variance
// of the centred block.  One workgroup (the block is at most a few MB); the sums are block_stats' (reduce.hpp).
template <typename T>
__global__ __launch_bounds__(1024)
void k_block_stats(const T* __restrict__ y, const T* __restrict__ fbar, int64_t n, int q, T* __restrict__ stats)
{
    __shared__ T red[16];
    __shared__ T smean[MAXQ];
    const T var = block_stats(y, fbar, n, q, red, smean);
    if (threadIdx.x == 0) {
        for (int c = 0; c < q; ++c) stats[c] = smean[c];
        stats[q] = var;
    }
}

template <typename T>
__global__ void k_residual(const T* __restrict__ y, const T* __restrict__ fbar, const T* __restrict__ bias,
                           int64_t total, int q, T* __restrict__ r)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % q);
    r[e] = y[e] - (fbar ? fbar[e] : (T)0) - (bias ? bias[c] : (T)0);
}

template <typename T>
__global__ void k_train_mean(const T* __restrict__ r, const T* __restrict__ alpha, const T* __restrict__ bias,
                             const T* __restrict__ noise, int64_t total, int q, T* __restrict__ out, int accumulate)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % q);
    const T v = r[e] - noise[0] * alpha[e] + (bias ? bias[c] : (T)0);
    out[e] = accumulate ? out[e] + v : v;
}

template <typename T>
__global__ void k_add_diag(T* __restrict__ k, int64_t n, int64_t ld, const T* __restrict__ noise)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) k[i * ld + i] += noise[0];
}

template <typename T>
__global__ void k_noise_from_stats(const T* __restrict__ stats, int q, T frac, T floor_value, T* __restrict__ noise)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const T v = frac * stats[q];
        noise[0] = (v > floor_value) ? v : floor_value;
    }
}

// sum_i log L_ii over one workgroup: thread t takes i = t, t + blockDim.x, ..; block_sum (reduce.hpp) adds.  Every
// thread returns the sum.  red: 16 doubles in LDS.
template <typename T>
static __device__ __forceinline__ double logdet_half(const T* __restrict__ l, int64_t n, int64_t ld, double* red)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += log((double)l[i * ld + i]);
    return block_sum(s, red);
}

template <typename T>
__global__ __launch_bounds__(1024)
void k_logdet_half(const T* __restrict__ l, int64_t n, int64_t ld, double* __restrict__ out)
{
    __shared__ double red[16];
    const double s = logdet_half(l, n, ld, red);
    if (threadIdx.x == 0) out[0] = s;
}

}  // namespace

template <typename T>
int misc_block_stats(const T* y, const T* fbar, int64_t n, int q, T* stats, hipStream_t st)
{
    const char* fn = "cimrgp_block_stats";
    CIMRGP_REQUIRE(n > 0, fn, "empty block");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    hipLaunchKernelGGL((k_block_stats<T>), dim3(1), dim3(1024), 0, st, y, fbar, n, q, stats);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int misc_residual(const T* y, const T* fbar, const T* bias, int64_t n, int q, T* r, hipStream_t st)
{
    const char* fn = "cimrgp_residual";
    if (n <= 0) return 0;
    CIMRGP_REQUIRE(q >= 1, fn, "q must be positive");
    const int64_t total = n * q;
    hipLaunchKernelGGL((k_residual<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, fbar, bias, total, q, r);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int misc_train_mean(const T* r, const T* alpha, const T* bias, const T* noise, int64_t n, int q, T* out,
                    int accumulate, hipStream_t st)
{
    const char* fn = "cimrgp_train_mean";
    if (n <= 0) return 0;
    CIMRGP_REQUIRE(q >= 1, fn, "q must be positive");
    const int64_t total = n * q;
    hipLaunchKernelGGL((k_train_mean<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       r, alpha, bias, noise, total, q, out, accumulate);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int misc_add_diag(T* k, int64_t n, int64_t ld, const T* noise, hipStream_t st)
{
    const char* fn = "cimrgp_add_diag";
    if (n <= 0) return 0;
    hipLaunchKernelGGL((k_add_diag<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, k, n, ld, noise);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int misc_noise_from_stats(const T* stats, int q, double frac, double floor_value, T* noise, hipStream_t st)
{
    const char* fn = "cimrgp_noise_from_stats";
    hipLaunchKernelGGL((k_noise_from_stats<T>), dim3(1), dim3(64), 0, st, stats, q, (T)frac, (T)floor_value, noise);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int misc_logdet_half(const T* l, int64_t n, int64_t ld, double* out, hipStream_t st)
{
    const char* fn = "cimrgp_logdet_half";
    CIMRGP_REQUIRE(n > 0, fn, "empty matrix");
    hipLaunchKernelGGL((k_logdet_half<T>), dim3(1), dim3(1024), 0, st, l, n, ld, out);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

#define CIMRGP_INST(T)                                                                                   \
    template int misc_block_stats<T>(const T*, const T*, int64_t, int, T*, hipStream_t);                 \
    template int misc_residual<T>(const T*, const T*, const T*, int64_t, int, T*, hipStream_t);          \
    template int misc_train_mean<T>(const T*, const T*, const T*, const T*, int64_t, int, T*, int, hipStream_t); \
    template int misc_add_diag<T>(T*, int64_t, int64_t, const T*, hipStream_t);                          \
    template int misc_noise_from_stats<T>(const T*, int, double, double, T*, hipStream_t);               \
    template int misc_logdet_half<T>(const T*, int64_t, int64_t, double*, hipStream_t);
CIMRGP_INST(double)
CIMRGP_INST(float)
#undef CIMRGP_INST

}  // namespace cimrgp

// ---------------------------------------------------------------------------
// Gradient of the log marginal likelihood (the `.optimize()` step of
// RegressionInput.py:63).  With G = alpha alpha^T - q K^-1 and the RBF parametrisation
// K = sf E + noise I,  E_ij = exp(-d2_ij / (2 l^2)):
//     dLML/dlog(sf)    = 1/2 sum_ij G_ij sf E_ij
//     dLML/dlog(l)     = 1/2 sum_ij G_ij sf E_ij d2_ij / l^2
//     dLML/dlog(noise) = 1/2 noise sum_i G_ii
// One pass over the LOWER triangle of K^-1 (off-diagonal entries count twice); the kernel
// matrix is re-evaluated on the fly from X, nothing n x n besides K^-1 is read.  Per-tile
// partial sums, then a fixed-order final reduction (deterministic).
// The Matern policies (common.hpp) replace sf E_ij by k_ij and sf E_ij d2_ij / l^2 by their
// d k / d log l: one kernel, k_lml_grad_tiles<T, COV, ARD>, whose RBF arm keeps the expressions above.
// ---------------------------------------------------------------------------
namespace cimrgp {
namespace {

constexpr int LG_T = 64;

// ARD: one length-scale per input dimension.  The caller passes inputs already divided by their
// length-scales (so the kernel is evaluated with l = 1) and gets d/dlog l_k = 1/2 sum G K d_k^2 per
// dimension: partial record = [sf | l_1 .. l_8 | trace] (LG_NP entries) instead of [sf | l | trace].
constexpr int LG_NP = MAXD + 2;

// BATCHED: blockIdx.y = block b of a layer (cimrgp_layer_lml_grad_cov): x from row starts[b], K^-1 at b * ks, alpha at
// b * n * q, the partial records at b * gridDim.x.  The single-block instance (BATCHED = false) reads none of these.
struct LgBatch { const int64_t* starts; int64_t ks; };
#define CIMRGP_LG_BLOCK(NP)                                 \
    if (BATCHED) {                                          \
        const int64_t b_ = blockIdx.y;                      \
        x += bb.starts[b_] * d;                             \
        kinv += b_ * bb.ks;                                 \
        alpha += b_ * (int64_t)n * q;                       \
        partial += b_ * (int64_t)gridDim.x * (NP);          \
    }

// c = cov_scale(COV, l); inv_l2 = 1 / l^2 is read by the RBF alone.
template <typename T, int COV, bool ARD, bool BATCHED = false>
__global__ __launch_bounds__(256)
void k_lml_grad_tiles(const T* __restrict__ x, int n, int d, const T* __restrict__ kinv, int64_t ld,
                      const T* __restrict__ alpha, int q, T c, T sf2, T inv_l2,
                      double* __restrict__ partial, LgBatch bb)
{
    CIMRGP_LG_BLOCK(ARD ? LG_NP : 3)
    __shared__ T sa[LG_T * MAXD], sb[LG_T * MAXD];
    __shared__ T aa[LG_T * 8], ab[LG_T * 8];
    __shared__ double red[ARD ? LG_NP : 3][4];
    const int id = blockIdx.x;
    int ti, tj;
    lower_tile_of(id, ti, tj);
    const int row0 = ti * LG_T, col0 = tj * LG_T;
    const int tid = threadIdx.x;
    for (int e = tid; e < LG_T * MAXD; e += 256) {
        const int r = e / MAXD, k = e - r * MAXD;
        sa[e] = (k < d && row0 + r < n) ? x[(int64_t)(row0 + r) * d + k] : (T)0;
        sb[e] = (k < d && col0 + r < n) ? x[(int64_t)(col0 + r) * d + k] : (T)0;
        aa[e] = (k < q && row0 + r < n) ? alpha[(int64_t)(row0 + r) * q + k] : (T)0;
        ab[e] = (k < q && col0 + r < n) ? alpha[(int64_t)(col0 + r) * q + k] : (T)0;
    }
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
    double s_sf = 0.0, s_l = 0.0, s_tr = 0.0;
    double s_lk[ARD ? MAXD : 1];
#pragma unroll
    for (int k = 0; k < (ARD ? MAXD : 1); ++k) s_lk[k] = 0.0;
    const int gc = col0 + tx;
    for (int rr = ty; rr < LG_T; rr += 4) {
        const int gr = row0 + rr;
        if (gr < n && gc < n && gc <= gr) {
            T d2 = (T)0;
            T dk2[MAXD];
#pragma unroll
            for (int k = 0; k < MAXD; ++k) {
                const T df = sa[rr * MAXD + k] - sb[tx * MAXD + k];
                dk2[k] = df * df;
                d2 += dk2[k];
            }
            T aat = (T)0;
#pragma unroll
            for (int k = 0; k < 8; ++k) aat += aa[rr * 8 + k] * ab[tx * 8 + k];
            const T g = aat - (T)q * kinv[(int64_t)gr * ld + gc];
            const double wgt = (gr == gc) ? 1.0 : 2.0;
            // kf = k_ij; gk dk2[k] = g dk_ij/dlog l_k (ARD); gl = g dk_ij/dlog l
            T kf, gk, gl;
            if constexpr (COV == CIMRGP_COV_RBF) {
                kf = sf2 * exp(d2 * c);
                // the RBF's own products, not pair()'s: (g kf) leads, and inv_l2 = 1 / l^2 is a factor rounded on its own
                gk = g * kf;
                gl = g * kf * d2 * inv_l2;
            } else {
                // r from d2 (a sum of squares: exactly 0 on the diagonal); d = 1 takes |df| as the Gram kernels do
                const T r = d == 1 ? fabs(sa[rr * MAXD] - sb[tx * MAXD]) : sqrt(d2);
                const T t = c * r, v = exp(-t);
                kf = sf2 * Cov<COV>::poly(t) * v;
                gk = g * Cov<COV>::ard(t, r, v, c, sf2);
                gl = g * Cov<COV>::dlogl(t, v, sf2);
            }
            s_sf += wgt * (double)(g * kf);
            if (ARD) {
#pragma unroll
                for (int k = 0; k < MAXD; ++k) s_lk[k] += wgt * (double)(gk * dk2[k]);
            } else {
                s_l  += wgt * (double)gl;
            }
            if (gr == gc) s_tr += (double)g;
        }
    }
    // the lanes of a wave by wave_sum, then the four waves' lane-0 values in wave order (sum4; reduce.hpp)
    if constexpr (ARD) wave_sum(s_sf, s_tr, s_lk);
    else               wave_sum(s_sf, s_l, s_tr);
    if (ARD) {
        if (tx == 0) {
            red[0][ty] = s_sf;
#pragma unroll
            for (int k = 0; k < MAXD; ++k) red[1 + k][ty] = s_lk[k];
            red[LG_NP - 1][ty] = s_tr;
        }
        __syncthreads();
        if (tid < LG_NP) partial[(int64_t)id * LG_NP + tid] = sum4(red[tid][0], red[tid][1], red[tid][2], red[tid][3]);
    } else {
        if (tx == 0) { red[0][ty] = s_sf; red[1][ty] = s_l; red[2][ty] = s_tr; }
        __syncthreads();
        if (tid < 3) partial[(int64_t)id * 3 + tid] = sum4(red[tid][0], red[tid][1], red[tid][2], red[tid][3]);
    }
}

// Entry c of the nout gradient entries from the tile records of one block, over one workgroup: np entries per record,
// the last one the trace term, which is the last gradient entry (the noise's); the first nout - 1 are taken as they
// come.  Thread t takes tiles t, t + blockDim.x, ..; block_sum (reduce.hpp) adds.  Every thread returns the entry.
static __device__ __forceinline__ double lml_grad_entry(const double* __restrict__ partial, int64_t ntiles, int np, int nout, int c,
                                                        double noise, double* red)
{
    const int src = (c == nout - 1) ? np - 1 : c;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < ntiles; t += blockDim.x) s += partial[t * np + src];
    s = block_sum(s, red);
    return 0.5 * s * (c == nout - 1 ? noise : 1.0);
}

__global__ __launch_bounds__(1024)
void k_lml_grad_final(const double* __restrict__ partial, int64_t ntiles, double noise, double* __restrict__ out,
                      int np, int nout)
{
    __shared__ double red[16];
    for (int c = 0; c < nout; ++c) {
        const double g = lml_grad_entry(partial, ntiles, np, nout, c, noise, red);
        if (threadIdx.x == 0) out[c] = g;
    }
}

}  // namespace

template <typename T, int COV>
static int lml_grad_run_cov(const T* x, int64_t n, int d, const T* kinv, int64_t ld, const T* alpha, int q,
                            double ell, double sf2, double noise, double* out3, double* scratch, hipStream_t st, bool ard,
                            const char* fn)
{
    CIMRGP_REQUIRE(n > 0 && n < (1ll << 30), fn, "bad size");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    const int64_t tm = (n + LG_T - 1) / LG_T, tiles = tm * (tm + 1) / 2;
    CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
    if (ard) {
        // inputs are pre-scaled by the length-scales: unit length-scale here; out = [sf | l_1..l_d | noise]
        hipLaunchKernelGGL((k_lml_grad_tiles<T, COV, true>), dim3((unsigned)tiles), dim3(256), 0, st, x, (int)n, d, kinv, ld, alpha, q,
                           (T)cov_scale(COV, 1.0), (T)sf2, (T)1, scratch, LgBatch{nullptr, 0});
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL(k_lml_grad_final, dim3(1), dim3(1024), 0, st, (const double*)scratch, tiles, noise, out3, LG_NP, d + 2);
    } else {
        hipLaunchKernelGGL((k_lml_grad_tiles<T, COV, false>), dim3((unsigned)tiles), dim3(256), 0, st, x, (int)n, d, kinv, ld, alpha, q,
                           (T)cov_scale(COV, ell), (T)sf2, (T)(1.0 / (ell * ell)), scratch, LgBatch{nullptr, 0});
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL(k_lml_grad_final, dim3(1), dim3(1024), 0, st, (const double*)scratch, tiles, noise, out3, 3, 3);
    }
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int lml_grad_run(const T* x, int64_t n, int d, const T* kinv, int64_t ld, const T* alpha, int q,
                 double ell, double sf2, double noise, double* out3, double* scratch, hipStream_t st, bool ard, int cov, const char* fn)
{
    if (!fn) fn = "cimrgp_lml_grad";
    return with_cov(cov, [&](auto c) {
        return lml_grad_run_cov<T, decltype(c)::value>(x, n, d, kinv, ld, alpha, q, ell, sf2, noise, out3, scratch, st, ard, fn);
    });
}

template int lml_grad_run<double>(const double*, int64_t, int, const double*, int64_t, const double*, int, double, double,
                                  double, double*, double*, hipStream_t, bool, int, const char*);
template int lml_grad_run<float>(const float*, int64_t, int, const float*, int64_t, const float*, int, double, double,
                                 double, double*, double*, hipStream_t, bool, int, const char*);

// ---- a layer's blocks at once (cimrgp_layer_lml_grad_cov) ----
// The tile kernels above with grid.y = block, then per block one workgroup that finishes it: the gradient from its
// tile records (lml_grad_entry, as k_lml_grad_final), the data fit sum_c z_c^T z_c = sum_c r_c^T K^-1 r_c from
// z = L^-1 r, and sum_i log L_ii from the factor's diagonal (logdet_half, as k_logdet_half):
//   out[4b + 0] = -1/2 fit - q sum log L_ii - 1/2 n q log 2 pi,  out[4b + 1 .. 3] = the gradient.
// ARD (cimrgp_layer_lml_grad_ard_cov): tile records of LG_NP entries and nout = d + 2 gradient entries, the record of
// block b at out[(d + 3) b]: [LML | sf | l_1 .. l_d | noise].  One body for both; per component the sums run in the
// same order whatever the record width.
namespace {

// NP entries per tile record, the last one the trace term; nout <= NP gradient entries, the last one the noise's
template <typename T, int NP>
__device__ __forceinline__
void layer_lml_final(const double* __restrict__ partial, int64_t ntiles, double noise, const T* __restrict__ l, int64_t ld,
                     int64_t ls, const T* __restrict__ z, int64_t n, int q, double* __restrict__ out, int nout)
{
    __shared__ double red[16];
    const int64_t b = blockIdx.x;
    partial += b * ntiles * NP;
    l += b * ls;
    z += b * n * q;
    double g[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        g[c] = c < nout ? lml_grad_entry(partial, ntiles, NP, nout, c, noise, red) : 0.0;
    }
    const double half_logdet = logdet_half(l, n, ld, red);
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < n * q; e += blockDim.x) s += (double)z[e] * (double)z[e];
    const double fit = block_sum(s, red);
    if (threadIdx.x == 0) {
        out[(nout + 1) * b + 0] = -0.5 * fit - (double)q * half_logdet - 0.5 * (double)(n * q) * log(2.0 * M_PI);
#pragma unroll
        for (int c = 0; c < NP; ++c)
            if (c < nout) out[(nout + 1) * b + 1 + c] = g[c];
    }
}

template <typename T>
__global__ __launch_bounds__(1024)
void k_layer_lml_final(const double* __restrict__ partial, int64_t ntiles, double noise, const T* __restrict__ l, int64_t ld,
                       int64_t ls, const T* __restrict__ z, int64_t n, int q, double* __restrict__ out)
{
    layer_lml_final<T, 3>(partial, ntiles, noise, l, ld, ls, z, n, q, out, 3);
}

template <typename T>
__global__ __launch_bounds__(1024)
void k_layer_lml_final_ard(const double* __restrict__ partial, int64_t ntiles, double noise, const T* __restrict__ l, int64_t ld,
                           int64_t ls, const T* __restrict__ z, int64_t n, int q, double* __restrict__ out, int nout)
{
    layer_lml_final<T, LG_NP>(partial, ntiles, noise, l, ld, ls, z, n, q, out, nout);
}

}  // namespace

int lml_grad_record_width(bool ard) { return ard ? LG_NP : 3; }

int64_t lml_grad_tiles_count(int64_t n)
{
    const int64_t tm = (n + LG_T - 1) / LG_T;
    return tm * (tm + 1) / 2;
}

template <typename T>
int lml_grad_batched_run(const T* x, const int64_t* starts, int batch, int64_t n, int d, const T* kinv, int64_t ld, int64_t ks,
                         const T* l, const T* alpha, const T* z, int q, double ell, double sf2, double noise, double* out,
                         double* partial, hipStream_t st, int cov, const char* fn, bool ard)
{
    CIMRGP_REQUIRE(n > 0 && n < (1ll << 30), fn, "bad size");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    const int64_t tiles = lml_grad_tiles_count(n);
    CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
    const LgBatch bb{starts, ks};
    const int rc = with_cov(cov, [&](auto c) {
        constexpr int COV = decltype(c)::value;
        if (ard)      // inputs pre-scaled by the length-scales: unit length-scale here, as in lml_grad_run_cov
            hipLaunchKernelGGL((k_lml_grad_tiles<T, COV, true, true>), dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, st, x,
                               (int)n, d, kinv, ld, alpha, q, (T)cov_scale(COV, 1.0), (T)sf2, (T)1, partial, bb);
        else
            hipLaunchKernelGGL((k_lml_grad_tiles<T, COV, false, true>), dim3((unsigned)tiles, (unsigned)batch), dim3(256), 0, st, x,
                               (int)n, d, kinv, ld, alpha, q, (T)cov_scale(COV, ell), (T)sf2, (T)(1.0 / (ell * ell)), partial, bb);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
    if (rc) return rc;
    if (ard)
        hipLaunchKernelGGL((k_layer_lml_final_ard<T>), dim3((unsigned)batch), dim3(1024), 0, st, (const double*)partial, tiles, noise, l,
                           ld, ks, z, n, q, out, d + 2);
    else
        hipLaunchKernelGGL((k_layer_lml_final<T>), dim3((unsigned)batch), dim3(1024), 0, st, (const double*)partial, tiles, noise, l, ld,
                           ks, z, n, q, out);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template int lml_grad_batched_run<double>(const double*, const int64_t*, int, int64_t, int, const double*, int64_t, int64_t,
                                          const double*, const double*, const double*, int, double, double, double, double*,
                                          double*, hipStream_t, int, const char*, bool);
template int lml_grad_batched_run<float>(const float*, const int64_t*, int, int64_t, int, const float*, int64_t, int64_t,
                                         const float*, const float*, const float*, int, double, double, double, double*,
                                         double*, hipStream_t, int, const char*, bool);

}  // namespace cimrgp
