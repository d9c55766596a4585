// What the psi statistics (psi.hip) and their gradients (psi_grad.hip) share: the compile-time dispatch over the input
// dimension, the slice rule of include/cimrgp_psi.h for any tile count, the enumeration of the lower triangle's tiles,
// and the exponential in the call's dtype.
#pragma once
#include "abi.hpp"

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

}  // namespace cimrgp
