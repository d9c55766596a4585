// What the psi statistics (psi.hip) and their gradients (psi_grad.hip) share: the compile-time dispatch over the input
// dimension, the slice rule of include/cimrgp_psi.h for any tile count, the enumeration of the lower triangle's tiles,
// the exponential in the call's dtype, and the pass over the rows that writes each row's constants.
#pragma once
#include "abi.hpp"
#include "reduce.hpp"

#include <math.h>

namespace cimrgp {

static __device__ __forceinline__ float t_exp(float x) { return expf(x); }
static __device__ __forceinline__ double t_exp(double x) { return exp(x); }

// the input dimension as a compile-time D = d exactly, 1 .. MAXD (validated by the entry points)
template <typename F> static inline auto with_dim_exact(int d, F&& f)
{
    switch (d) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        case 7: return f(std::integral_constant<int, 7>());
        default: return f(std::integral_constant<int, 8>());
    }
}

static inline int64_t round16(int64_t b) { return (b + 15) / 16 * 16; }

// tiles of `edge` x `edge` pairs per side of an m x m matrix, and in its lower triangle
static inline int64_t psi_tiles_1d(int64_t m, int64_t edge) { return (m + edge - 1) / edge; }
static inline int64_t psi_tiles(int64_t m, int64_t edge) { const int64_t t = psi_tiles_1d(m, edge); return t * (t + 1) / 2; }

// The slice rule of include/cimrgp_psi.h for `units` workgroups per slice: the slice length, so that units x slices is
// about `target` workgroups and no slice is shorter than CIMRGP_PSI2_MIN_SLICE rows.  A function of its arguments alone.
static inline int64_t psi_slice_len(int64_t n, int64_t units, int64_t target)
{
    int64_t s = target / units;
    const int64_t smax = (n + CIMRGP_PSI2_MIN_SLICE - 1) / CIMRGP_PSI2_MIN_SLICE;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int64_t len = (n + s - 1) / s;
    return (len + CIMRGP_PSI2_SLICE_ALIGN - 1) / CIMRGP_PSI2_SLICE_ALIGN * CIMRGP_PSI2_SLICE_ALIGN;
}
static inline int64_t psi_slice_count(int64_t n, int64_t len) { return (n + len - 1) / len; }

static inline bool psi2_sizes_ok(int64_t n, int64_t m) { return n >= 1 && n <= CIMRGP_PSI2_MAX_N && m >= 1 && m <= CIMRGP_PSI2_MAX_M; }

// one count of bad rows per 256 rows (float64), a multiple of 16 bytes
static inline int64_t psi2_count_blocks(int64_t n) { return (n + 255) / 256; }
static inline int64_t psi2_count_bytes(int64_t n) { return round16(psi2_count_blocks(n) * 8); }

// tile number -> (ti, tj), tj <= ti: column tj of the triangle holds tiles1d - tj tiles, the diagonal one first
static __device__ __forceinline__ void psi2_tile_of(int tile, int tiles1d, int& ti, int& tj)
{
    int first = 0;
    tj = 0;
    while (tile >= first + (tiles1d - tj)) { first += tiles1d - tj; ++tj; }
    ti = tj + (tile - first);
}

namespace {

// The pass over the rows that cimrgp_psi2 and cimrgp_psi2_rows_quad start with.
// rc[i] = (mu_i0 .. mu_i,D-1, r_i0 .. r_i,D-1, c0_i); badpart[blockIdx.x] = the workgroup's count of bad rows.
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2_rows(const T* __restrict__ mu, const T* __restrict__ s, int n, const double* __restrict__ ell, T* __restrict__ rc,
                 double* __restrict__ badpart)
{
    constexpr int RS = 2 * D + 1;
    __shared__ double red[16];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    double bad = 0.0;
    if (i < n) {
        T o[RS];
        double lg = 0.0;
        bool ok = true;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const double sv = (double)s[(int64_t)i * D + e], l2 = ell[e] * ell[e];
            ok = ok && sv >= 0.0 && sv - sv == 0.0;              // not negative, not NaN, not infinite
            o[e] = mu[(int64_t)i * D + e];
            o[D + e] = (T)(1.0 / (l2 + 2.0 * sv));
            lg += log1p(2.0 * sv / l2);
        }
        o[2 * D] = (T)(-0.5 * lg);
        if (!ok) {
            bad = 1.0;
#pragma unroll
            for (int k = 0; k < 2 * D; ++k) o[k] = (T)0;
            o[2 * D] = -(T)INFINITY;
        }
#pragma unroll
        for (int k = 0; k < RS; ++k) rc[(int64_t)i * RS + k] = o[k];
    }
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) badpart[blockIdx.x] = bad;
}

}  // namespace

}  // namespace cimrgp
