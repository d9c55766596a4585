// D1: tiled Gram / cross-Gram builder and D4: fused predictive mean.  One kernel template per operation, every one
// with the covariance policy COV of common.hpp (CIMRGP_COV_*: RBF = 0, Matern 1/2, 3/2, 5/2) as a parameter:
// k_gram<T, COV, SYMM, D> (and k_gram_lin, its arm with a linear term), k_gram_lower_wide<T, COV, D>, k_gram_batched<T, COV, SYMM, D>, k_predict_mean<T, COV, D, Q>.
//
// Gram: one workgroup = one 64 x 64 tile; the row and column input tiles are
// staged in LDS once; each thread produces a 4 x 4 patch whose 4 columns are
// contiguous, so a 16-lane row group stores 16 x 32 B (f64) = 512 contiguous
// bytes per matrix row.  HBM-write bound: n^2 * sizeof(T) bytes,
// with the exp as the secondary limiter in f64.
#include "common.hpp"

namespace cimrgp {

namespace {

constexpr int GTILE = 64;

// What a lane does with a staged tile of GTILE rows (sa) and WIDTH columns (sb) at (row0, col0): its part of every row.
// D = compile-time input dimension (1, 2) or 0 = run-time d <= 8 with fully
// unrolled, predicated loops (run-time indexed register arrays would spill).
// SYMM: diag_add on the diagonal; SKIP: lanes whose columns lie right of the tile's last row do nothing.
//
// Store layout (round 3): a lane owns the 16 bytes it stores with ONE instruction -- EPL = 2 doubles / 4 floats
// of one row -- and the lanes of a wave are adjacent along the row: every store instruction writes whole
// 512-byte runs (WIDTH = 64: 2 rows x 32 lanes in FP64, 4 rows x 16 lanes in FP32).  (Rounds 1-2: 4 adjacent columns =
// 32 bytes per lane in two instructions, each of which wrote every other 16 bytes of its run: 3.5 TB/s with
// the exponential taken out, against 5.8 TB/s for a plain fill of the same bytes.)
//
// LIN (include/cimrgp_sparse_linear.h): every element gets + sum_e lin[e] xa_ie xb_je.  The lane keeps lin[e] xb_je of its
// EPL columns beside xc, rounded to the dtype once; an element costs d more multiply-adds in the dtype.  Nothing else
// changes: the store layout is the one above.
template <typename T, int COV, bool SYMM, int D, int WIDTH, bool SKIP, bool LIN = false>
static __device__ __forceinline__ void gram_lanes(const T* sa, const T* sb, int row0, int col0, int na, int nb, int d,
                                                   T c, T sf2, T diag_add, T* __restrict__ K, int64_t ld,
                                                   const double* __restrict__ lin = nullptr)
{
    constexpr int EPL = 16 / (int)sizeof(T);    // elements per lane and row
    constexpr int LPR = WIDTH / EPL;            // lanes per tile row
    constexpr int RPI = 64 / LPR;               // rows per wave and store instruction
    constexpr int NIT = GTILE / (4 * RPI);      // row iterations: 4 waves x RPI rows each
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cx = (lane % LPR) * EPL;          // first column of this lane inside the tile
    const int ry = lane / LPR;                  // row of this lane inside a wave's row group
    const int gc = col0 + cx;
    if (SKIP && gc > row0 + GTILE - 1) return;  // (behind the only barrier) all of this lane's columns are above the diagonal in every row of the tile
    constexpr int DD = D ? D : MAXD;
    T xc[EPL][DD];
#pragma unroll
    for (int b = 0; b < EPL; ++b)
#pragma unroll
        for (int k = 0; k < DD; ++k) xc[b][k] = sb[(cx + b) * MAXD + k];
    T xl[LIN ? EPL : 1][LIN ? DD : 1];
    if constexpr (LIN) {
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            const T w = (D || k < d) ? (T)lin[k] : (T)0;
#pragma unroll
            for (int b = 0; b < EPL; ++b) xl[b][k] = w * xc[b][k];
        }
    }

#pragma unroll
    for (int a = 0; a < NIT; ++a) {
        const int r  = (a * 4 + wave) * RPI + ry;
        const int gr = row0 + r;
        if (gr >= na) continue;
        T out[EPL];
#pragma unroll
        for (int b = 0; b < EPL; ++b) {
            // k(x, x') of policy COV (c = cov_scale(COV, l)); df0, the first difference, gives r = |df0| when D = 1
            T d2 = (T)0, df0 = (T)0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (D || k < d) {
                    const T df = sa[r * MAXD + k] - xc[b][k];
                    if (COV != CIMRGP_COV_RBF && k == 0) df0 = df;
                    d2 += df * df;
                }
            }
            T v = Cov<COV>::template value<T, D>(d2, df0, c, sf2);
            if constexpr (LIN) {
                T dot = (T)0;
#pragma unroll
                for (int k = 0; k < DD; ++k)
                    if (D || k < d) dot += sa[r * MAXD + k] * xl[b][k];
                v += dot;
            }
            if (SYMM && (gr == gc + b)) v += diag_add;
            out[b] = v;
        }
        T* dst = K + (int64_t)gr * ld + gc;
        if (gc + EPL - 1 < nb && ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0)) {
            // non-temporal: the matrix is written once and read next by another kernel (round 4: 65.5 -> 59-61 us at
            // n = 8192, lower tiles)
            typedef double d2v __attribute__((ext_vector_type(2)));
            typedef float f4v __attribute__((ext_vector_type(4)));
            if (sizeof(T) == 8) { d2v v = {(double)out[0], (double)out[1]}; __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(dst)); }
            else { f4v v = {(float)out[0], (float)out[1], (float)out[EPL - 2], (float)out[EPL - 1]}; __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(dst)); }
        } else {
#pragma unroll
            for (int b = 0; b < EPL; ++b)
                if (gc + b < nb) dst[b] = out[b];
        }
    }
}

// One 64 x 64 tile of k(xa, xb): tile blockIdx.x of the tiles_n per tile row, or (SYMM, lower_only) of the lower triangle
template <typename T, int COV, bool SYMM, int D, bool LIN = false>
static __device__ __forceinline__ void gram_tile(const T* __restrict__ xa, int na, const T* __restrict__ xb, int nb, int d,
                                                  T c, T sf2, T diag_add, T* __restrict__ K, int64_t ld,
                                                  int tiles_n, int lower_only, const double* __restrict__ lin = nullptr)
{
    __shared__ T sa[GTILE * MAXD];
    __shared__ T sb[GTILE * MAXD];
    int ti, tj;
    if (SYMM && lower_only) {
        lower_tile_of(blockIdx.x, ti, tj);
    } else {
        ti = blockIdx.x / tiles_n;
        tj = blockIdx.x - ti * tiles_n;
    }
    const int row0 = ti * GTILE, col0 = tj * GTILE;
    for (int e = threadIdx.x; e < GTILE * MAXD; e += 256) {
        const int r = e / MAXD, k = e - r * MAXD;
        sa[e] = (k < d && row0 + r < na) ? xa[(int64_t)(row0 + r) * d + k] : (T)0;
        sb[e] = (k < d && col0 + r < nb) ? xb[(int64_t)(col0 + r) * d + k] : (T)0;
    }
    __syncthreads();
    gram_lanes<T, COV, SYMM, D, GTILE, false, LIN>(sa, sb, row0, col0, na, nb, d, c, sf2, diag_add, K, ld, lin);
}

template <typename T, int COV, bool SYMM, int D>
__global__ __launch_bounds__(256)
void k_gram(const T* __restrict__ xa, int na, const T* __restrict__ xb, int nb, int d,
            T c, T sf2, T diag_add, T* __restrict__ K, int64_t ld, int tiles_n, int lower_only)
{
    gram_tile<T, COV, SYMM, D>(xa, na, xb, nb, d, c, sf2, diag_add, K, ld, tiles_n, lower_only);
}

// The LIN arm of k_gram: lin = d FP64 weights on the device (both dtypes).
template <typename T, int COV, bool SYMM, int D>
__global__ __launch_bounds__(256)
void k_gram_lin(const T* __restrict__ xa, int na, const T* __restrict__ xb, int nb, int d,
                T c, T sf2, T diag_add, T* __restrict__ K, int64_t ld, int tiles_n, int lower_only, const double* __restrict__ lin)
{
    gram_tile<T, COV, SYMM, D, true>(xa, na, xb, nb, d, c, sf2, diag_add, K, ld, tiles_n, lower_only, lin);
}

// The lower triangle of a symmetric Gram matrix in 64 x 128 tiles (round 5): a tile row is 128 columns = 1 KB in FP64, so
// every store instruction of a wave writes ONE whole 1-KB run of one matrix row (FP32: two 512-byte runs); tile rows 2p
// and 2p+1 both need p + 1 tiles, so pair p starts at tile p (p + 1).  In the tile that holds the diagonal, lanes whose
// columns lie right of the tile's last row have nothing below the diagonal and skip.
constexpr int GWIDE = 128;
template <typename T, int COV, int D>
__global__ __launch_bounds__(256)
void k_gram_lower_wide(const T* __restrict__ x, int n, int d, T c, T sf2, T diag_add, T* __restrict__ K, int64_t ld)
{
    __shared__ T sa[GTILE * MAXD];
    __shared__ T sb[GWIDE * MAXD];
    const int id = blockIdx.x;
    int p = (int)((sqrtf(4.0f * (float)id + 1.0f) - 1.0f) * 0.5f);
    while (p * (p + 1) > id) --p;
    while ((p + 1) * (p + 2) <= id) ++p;
    const int rem = id - p * (p + 1);
    const int odd = rem >= p + 1;
    const int ti = 2 * p + odd, tj = rem - odd * (p + 1);
    const int row0 = ti * GTILE, col0 = tj * GWIDE;
    for (int e = threadIdx.x; e < GWIDE * MAXD; e += 256) {
        const int r = e / MAXD, k = e - r * MAXD;
        if (r < GTILE) sa[e] = (k < d && row0 + r < n) ? x[(int64_t)(row0 + r) * d + k] : (T)0;
        sb[e] = (k < d && col0 + r < n) ? x[(int64_t)(col0 + r) * d + k] : (T)0;
    }
    __syncthreads();
    gram_lanes<T, COV, true, D, GWIDE, true>(sa, sb, row0, col0, n, n, d, c, sf2, diag_add, K, ld);
}

// The blocks of one layer in one launch (blockIdx.y = block): block b takes its `na` rows of inputs at
// row a_starts[b] of xa and its `nb` columns at row b_starts[b] of xb (regions are contiguous ranges of
// the layer's arrays, Inputs.py:57-60), writes matrix b of the arena (stride kstride) and, on the
// diagonal of a symmetric matrix, adds ITS noise (diag_dev[b]).
template <typename T, int COV, bool SYMM, int D>
__global__ __launch_bounds__(256)
void k_gram_batched(const T* __restrict__ xa, const int64_t* __restrict__ a_starts, int na,
                    const T* __restrict__ xb, const int64_t* __restrict__ b_starts, int nb, int d,
                    T c, T sf2, const T* __restrict__ diag_dev, T* __restrict__ K, int64_t ld,
                    int64_t kstride, int tiles_n, int lower_only)
{
    const int b = blockIdx.y;
    gram_tile<T, COV, SYMM, D>(xa + a_starts[b] * d, na, xb + b_starts[b] * d, nb, d, c, sf2,
                               diag_dev ? diag_dev[b] : (T)0, K + (int64_t)b * kstride, ld, tiles_n, lower_only);
}

// D4: mean[i][c] (+)= bias[c] + sum_j k(xs_i, x_j) alpha[j][c], k of policy COV (cs = cov_scale(COV, l)).
// Workgroup = 8 test points x 32 partial sums over the training points; the
// cross-Gram row is never written anywhere.  Deterministic (fixed-order LDS
// reduction, no atomics).
constexpr int PM_TS = 8;
constexpr int PM_PH = 32;

// Q = number of outputs at compile time (a run-time guard inside the loop serialises the loads).
template <typename T, int COV, int D, int Q>
__global__ __launch_bounds__(256)
void k_predict_mean(const T* __restrict__ x, int n, int d, const T* __restrict__ alpha, int q,
                    const T* __restrict__ xs, int ns, T cs, T sf2,
                    const T* __restrict__ bias, T* __restrict__ mean, int accumulate)
{
    __shared__ T red[PM_PH][PM_TS][Q];
    const int tid = threadIdx.x;
    const int t  = tid & (PM_TS - 1);
    const int ph = tid / PM_TS;
    const int gi = blockIdx.x * PM_TS + t;
    constexpr int DD = D ? D : MAXD;
    T xt[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) xt[k] = ((D || k < d) && gi < ns) ? xs[(int64_t)gi * d + k] : (T)0;
    T sum[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) sum[c] = (T)0;
    for (int j = ph; j < n; j += PM_PH) {
        T d2 = (T)0, df0 = (T)0;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (D || k < d) {
                const T df = xt[k] - x[(int64_t)j * d + k];
                if (COV != CIMRGP_COV_RBF && k == 0) df0 = df;
                d2 += df * df;
            }
        }
        const T kv = Cov<COV>::template value<T, D>(d2, df0, cs, sf2);
#pragma unroll
        for (int c = 0; c < Q; ++c) sum[c] += kv * alpha[(int64_t)j * Q + c];
    }
#pragma unroll
    for (int c = 0; c < Q; ++c) red[ph][t][c] = sum[c];
    __syncthreads();
    if (tid < PM_TS * q) {
        const int tt = tid / q, c = tid - tt * q;
        const int g = blockIdx.x * PM_TS + tt;
        if (g < ns) {
            T s = bias ? bias[c] : (T)0;
            for (int p = 0; p < PM_PH; ++p) s += red[p][tt][c];
            T* o = mean + (int64_t)g * q + c;
            *o = accumulate ? (*o + s) : s;
        }
    }
}

}  // namespace

template <typename T, int COV>
static int gram_run_cov(const T* xa, int64_t na, const T* xb, int64_t nb, int d, double ell, double sf2,
                        double diag_add, T* k, int64_t ld, bool symm, bool lower_only, hipStream_t st, const char* fn, const double* lin)
{
    if (na <= 0 || nb <= 0) return 0;
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0, fn, "length-scale must be positive");
    CIMRGP_REQUIRE(ld >= nb, fn, "leading dimension smaller than the number of columns");
    CIMRGP_REQUIRE(na < (1ll << 30) && nb < (1ll << 30), fn, "matrix too large");
    const int64_t tm = (na + GTILE - 1) / GTILE, tn = (nb + GTILE - 1) / GTILE;
    const T c = (T)cov_scale(COV, ell);
    // the 64 x 64 tiles; with the linear term (lin != nullptr) the only form: K_uu is m x m
    auto launch = [&](auto symm_, int64_t tiles, double diag, int lo) {
        with_dim(d, [&](auto dd) {
            if (lin)
                hipLaunchKernelGGL((k_gram_lin<T, COV, decltype(symm_)::value, decltype(dd)::value>), dim3((unsigned)tiles), dim3(256), 0,
                                   st, xa, (int)na, xb, (int)nb, d, c, (T)sf2, (T)diag, k, ld, (int)tn, lo, lin);
            else
                hipLaunchKernelGGL((k_gram<T, COV, decltype(symm_)::value, decltype(dd)::value>), dim3((unsigned)tiles), dim3(256), 0, st,
                                   xa, (int)na, xb, (int)nb, d, c, (T)sf2, (T)diag, k, ld, (int)tn, lo);
        });
    };
    if (symm && lower_only && na == nb && xa == xb && !lin) {
        // the lower triangle in 64 x 128 tiles: pairs of tile rows, P (P + 1) tiles in the full pairs (+ P + 1 for an odd last row)
        const int64_t pairs = tm / 2;
        const int64_t tiles = pairs * (pairs + 1) + ((tm & 1) ? pairs + 1 : 0);
        CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
        with_dim(d, [&](auto dd) {
            hipLaunchKernelGGL((k_gram_lower_wide<T, COV, decltype(dd)::value>), dim3((unsigned)tiles), dim3(256), 0, st,
                               xa, (int)na, d, c, (T)sf2, (T)diag_add, k, ld);
        });
    } else if (symm) {
        const int64_t tiles = lower_only ? tm * (tm + 1) / 2 : tm * tn;
        CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
        launch(std::true_type(), tiles, diag_add, lower_only ? 1 : 0);
    } else {
        const int64_t tiles = tm * tn;
        CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
        launch(std::false_type(), tiles, 0.0, 0);
    }
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int rbf_gram_run(const T* xa, int64_t na, const T* xb, int64_t nb, int d, double ell, double sf2,
                 double diag_add, T* k, int64_t ld, bool symm, bool lower_only, hipStream_t st, int cov, const char* fn, const double* lin)
{
    if (!fn) fn = symm ? "cimrgp_rbf_gram" : "cimrgp_rbf_cross";
    return with_cov(cov, [&](auto c) {
        return gram_run_cov<T, decltype(c)::value>(xa, na, xb, nb, d, ell, sf2, diag_add, k, ld, symm, lower_only, st, fn, lin);
    });
}

template <typename T, int COV>
static int gram_batched_run_cov(const BatchCov& bc, const Points<T>& rows, const Points<T>& cols, const T* diag_dev, const Arena<T>& k,
                                bool symm, hipStream_t st)
{
    const char* fn = "cimrgp_layer";
    const int64_t na = rows.n, nb = cols.n;
    const int d = bc.d;
    if (na <= 0 || nb <= 0 || bc.batch <= 0) return 0;
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(bc.ell > 0.0, fn, "length-scale must be positive");
    CIMRGP_REQUIRE(k.ld >= nb, fn, "leading dimension smaller than the number of columns");
    CIMRGP_REQUIRE(na < (1ll << 30) && nb < (1ll << 30) && bc.batch < 65536, fn, "batch too large");
    const int64_t tm = (na + GTILE - 1) / GTILE, tn = (nb + GTILE - 1) / GTILE;
    const int64_t tiles = symm ? tm * (tm + 1) / 2 : tm * tn;
    CIMRGP_REQUIRE(tiles < (1ll << 31), fn, "grid too large");
    const T c = (T)cov_scale(COV, bc.ell);
    auto launch = [&](auto symm_) {
        with_dim(d, [&](auto dd) {
            hipLaunchKernelGGL((k_gram_batched<T, COV, decltype(symm_)::value, decltype(dd)::value>), dim3((unsigned)tiles, (unsigned)bc.batch),
                               dim3(256), 0, st, rows.x, rows.starts, (int)na, cols.x, cols.starts, (int)nb, d, c, (T)bc.sf2, diag_dev, k.p,
                               k.ld, k.stride, (int)tn, decltype(symm_)::value ? 1 : 0);
        });
    };
    if (symm) launch(std::true_type()); else launch(std::false_type());
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int rbf_gram_batched_run(const BatchCov& bc, const Points<T>& rows, const Points<T>& cols, const T* diag_dev, const Arena<T>& k, bool symm,
                         hipStream_t st)
{
    return with_cov(bc.cov, [&](auto c) { return gram_batched_run_cov<T, decltype(c)::value>(bc, rows, cols, diag_dev, k, symm, st); });
}

template <typename T, int COV>
static int predict_mean_run_cov(const T* x, int64_t n, int d, const T* alpha, int q, const T* xs, int64_t ns,
                                double ell, double sf2, const T* bias, T* mean, int accumulate, hipStream_t st, const char* fn)
{
    if (ns <= 0) return 0;
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0, fn, "length-scale must be positive");
    CIMRGP_REQUIRE(n < (1ll << 31) && ns < (1ll << 31), fn, "too many points");
    const unsigned grid = (unsigned)((ns + PM_TS - 1) / PM_TS);
    with_q(q, [&](auto qq) {
        with_dim(d, [&](auto dd) {
            hipLaunchKernelGGL((k_predict_mean<T, COV, decltype(dd)::value, decltype(qq)::value>), dim3(grid), dim3(256), 0, st, x, (int)n, d,
                               alpha, q, xs, (int)ns, (T)cov_scale(COV, ell), (T)sf2, bias, mean, accumulate);
        });
    });
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
int predict_mean_run(const T* x, int64_t n, int d, const T* alpha, int q, const T* xs, int64_t ns,
                     double ell, double sf2, const T* bias, T* mean, int accumulate, hipStream_t st, int cov, const char* fn)
{
    if (!fn) fn = "cimrgp_predict_mean";
    return with_cov(cov, [&](auto c) {
        return predict_mean_run_cov<T, decltype(c)::value>(x, n, d, alpha, q, xs, ns, ell, sf2, bias, mean, accumulate, st, fn);
    });
}

template int rbf_gram_run<double>(const double*, int64_t, const double*, int64_t, int, double, double, double,
                                  double*, int64_t, bool, bool, hipStream_t, int, const char*, const double*);
template int rbf_gram_run<float>(const float*, int64_t, const float*, int64_t, int, double, double, double,
                                 float*, int64_t, bool, bool, hipStream_t, int, const char*, const double*);
template int rbf_gram_batched_run<double>(const BatchCov&, const Points<double>&, const Points<double>&, const double*,
                                          const Arena<double>&, bool, hipStream_t);
template int rbf_gram_batched_run<float>(const BatchCov&, const Points<float>&, const Points<float>&, const float*,
                                         const Arena<float>&, bool, hipStream_t);
template int predict_mean_run<double>(const double*, int64_t, int, const double*, int, const double*, int64_t,
                                      double, double, const double*, double*, int, hipStream_t, int, const char*);
template int predict_mean_run<float>(const float*, int64_t, int, const float*, int, const float*, int64_t,
                                     double, double, const float*, float*, int, hipStream_t, int, const char*);

}  // namespace cimrgp
