// What the psi sources (psi.hip, psi_grad.hip, psi_rows.hip) share, each piece stated once: the dispatch over the input
// dimension, the slice rule and the tile enumeration, the reduce kernels' two fixed-order sums, the row constants and
// exponents of Psi1 and Psi2, the LDS stagings, a thread's points of a pair tile and the pass over the rows.
// Every hand-over through LDS is: stores, lds_settle on the last word stored, barrier (common.hpp).
#pragma once
#include "abi.hpp"
#include "reduce.hpp"

#include <math.h>

namespace cimrgp {

constexpr int PSI_TILE = CIMRGP_PSI2_TILE;          // tile edge (pairs) of cimrgp_psi2 and of the row-owning kernels
constexpr int PSI_CHUNK = 64;                    // rows whose constants are staged at a time

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

// the scratch parts every Psi2 call starts with, each a multiple of 16 bytes: one count of bad rows per 256 rows
// (float64), then the rows' constants, 2 d + 1 per row or 3 d + 1 for the gradient
static inline int64_t psi2_count_blocks(int64_t n) { return (n + 255) / 256; }
static inline int64_t psi2_count_bytes(int64_t n) { return round16(psi2_count_blocks(n) * 8); }
static inline int64_t psi2_rows_bytes(int dtype, int64_t n, int d, bool grad = false)
{
    return round16(n * ((grad ? 3 : 2) * d + 1) * (int64_t)elem_bytes(dtype));
}

// tile number -> (ti, tj), tj <= ti: column tj of the triangle holds tiles1d - tj tiles, the diagonal one first
static __device__ __forceinline__ void psi2_tile_of(int tile, int tiles1d, int& ti, int& tj)
{
    int first = 0;
    tj = 0;
    while (tile >= first + (tiles1d - tj)) { first += tiles1d - tj; ++tj; }
    ti = tj + (tile - first);
}

// ------------------------------------------------------ the reduce kernels' sums ----
// part[0] + part[stride] + .. + part[(count - 1) stride], ascending from the first partial: the order is the contract
template <typename T>
static __device__ __forceinline__ T psi_ordered_sum(const T* __restrict__ part, int count, int64_t stride)
{
    T acc = part[0];
    for (int p = 1; p < count; ++p) acc += part[(int64_t)p * stride];
    return acc;
}

// bad[0] = the number of bad rows: thread t adds badpart[t], [t + 256], .., then lds_tree (red: 256 elements)
static __device__ __forceinline__ void psi2_count_bad(const double* __restrict__ badpart, int nbad, double* red, int tid,
                                                      double* __restrict__ bad)
{
    double b = 0.0;
    for (int i = tid; i < nbad; i += 256) b += badpart[i];
    red[tid] = b;
    lds_tree<256>(red, tid);
    if (tid == 0) bad[0] = red[0];
}

// ----------------------------------------------------------------------- Psi1 ----
// One row's constants in float64, rounded once: mv[e] = mu_e, hr[e] = 1 / (2 (l_e^2 + s_e)), with SH also
// sh[e] = s_e / (l_e^2 + s_e); returns c0 = -1/2 sum log1p(s_e / l_e^2).
template <typename T, int D, bool SH = false>
static __device__ __forceinline__ T psi1_row_consts(const T* __restrict__ mu, const T* __restrict__ s, int64_t row,
                                                    const double* __restrict__ ell, T* mv, T* hr, T* sh = nullptr)
{
    double lg = 0.0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const double sv = (double)s[row * D + e], l2 = ell[e] * ell[e];
        mv[e] = mu[row * D + e];
        hr[e] = (T)(0.5 / (l2 + sv));
        if constexpr (SH) sh[e] = (T)(sv / (l2 + sv));
        lg += log1p(sv / l2);
    }
    return (T)(-0.5 * lg);
}

// c0 - sum_e (mu_e - z_e)^2 h_e; df[e] = mu_e - z_e for a caller that goes on with it
template <typename T, int D>
static __device__ __forceinline__ T psi1_exponent(T c0, const T* mv, const T* z, const T* hr, T* df)
{
    T ex = c0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        df[e] = mv[e] - z[e];
        ex = fma(-(df[e] * df[e]), hr[e], ex);
    }
    return ex;
}

template <typename T, int D> static __device__ __forceinline__ T psi1_exponent(T c0, const T* mv, const T* z, const T* hr)
{
    T df[D];
    return psi1_exponent<T, D>(c0, mv, z, hr, df);
}

// ----------------------------------------------------------------------- Psi2 ----
// The exponent in its direct form, c0 - sum_e ((mu_e - z_je / 2) - z_ke / 2)^2 r_e, with z / 2 held per point (halving is
// exact) and (z_j + z_k) / 2 never held per pair: the expanded form 1/2 (mu - z_j)^2 + 1/2 (mu - z_k)^2 - 1/4 (z_j - z_k)^2
// cancels when z_j and z_k are far apart with mu between them.  di[e] = mu_e - z_je / 2, hzk[e] = z_ke / 2, r[e] = r_e;
// with WANT_Q, q[e] = dl_e r_e.
template <typename T, int D, bool WANT_Q>
static __device__ __forceinline__ T psi2_exponent(T c0, const T* di, const T* hzk, const T* r, T* q = nullptr)
{
    T ex = c0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const T dl = di[e] - hzk[e];
        ex = fma(-(dl * dl), r[e], ex);
        if constexpr (WANT_Q) q[e] = dl * r[e];
    }
    return ex;
}

// The row-owning kernels (a thread per row: k_psi2g_rowpass, k_psi2rq_pass).  A thread's own constants from rc (RS per
// row, c0 last): mv, rv, and il2[e] = 1 / l_e^2; returns c0.  A thread past the last row gets (0, 0, -inf).
// c0 is read last: read ahead of the loop, k_psi2g_rowpass<float, 1> fuses three multiply-adds fewer than the parent.
template <typename T, int D, int RS>
static __device__ __forceinline__ T psi2_own_row(const T* __restrict__ rc, int i, bool live, const double* __restrict__ ell,
                                                 T (&mv)[D], T (&rv)[D], T (&il2)[D])
{
#pragma unroll
    for (int e = 0; e < D; ++e) {
        mv[e] = live ? rc[(int64_t)i * RS + e] : (T)0;
        rv[e] = live ? rc[(int64_t)i * RS + D + e] : (T)0;
        il2[e] = (T)(1.0 / (ell[e] * ell[e]));
    }
    return live ? rc[(int64_t)i * RS + RS - 1] : -(T)INFINITY;
}

// z / 2 of a tile's PSI_TILE + PSI_TILE points into LDS (zeros past m), settled; the caller's barriers stand around it
template <typename T, int D>
static __device__ __forceinline__ void psi2_stage_points(const T* __restrict__ z, int m, int i0, int j0, T* hzi, T* hzj, int tid)
{
    for (int idx = tid; idx < PSI_TILE * D; idx += 256) {
        const int gi = i0 + idx / D, gj = j0 + idx / D, e = idx % D;
        hzi[idx] = gi < m ? (T)0.5 * z[(int64_t)gi * D + e] : (T)0;
        hzj[idx] = gj < m ? (T)0.5 * z[(int64_t)gj * D + e] : (T)0;
        if (idx + 256 >= PSI_TILE * D) lds_settle(hzj + idx);
    }
}

// The pair-owning kernels (k_psi2_tiles, k_psi2g_pairs).  `words` row constants from global memory to LDS by the 256
// threads: barrier (the previous chunk has been read), stores, settle, barrier.
template <typename T>
static __device__ __forceinline__ void psi2_stage_chunk(T* lds, const T* __restrict__ src, int words, int tid)
{
    __syncthreads();
    for (int idx = tid; idx < words; idx += 256) {
        lds[idx] = src[idx];
        if (idx + 256 >= words) lds_settle(lds + idx);
    }
    __syncthreads();
}

// z / 2 of thread (ty, tx)'s PR + PR points of the tile at (i0, j0): i0 + ty + 16 a and j0 + tx + 16 a (zeros past m)
template <typename T, int D, int PR, bool FULL>
static __device__ __forceinline__ void psi2_pair_points(const T* __restrict__ z, int m, int i0, int j0, int ty, int tx,
                                                        T (&hzi)[PR][D], T (&hzj)[PR][D])
{
#pragma unroll
    for (int a = 0; a < PR; ++a) {
        const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * a;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            hzi[a][e] = (FULL || gi < m) ? (T)0.5 * z[(int64_t)gi * D + e] : (T)0;
            hzj[a][e] = (FULL || gj < m) ? (T)0.5 * z[(int64_t)gj * D + e] : (T)0;
        }
    }
}

namespace {

// The pass over the rows that every Psi2 call starts with: a thread per row, the constants in float64, rounded once.
// rc[i] = (mu_i0 .., r_i0 .., c0_i), r = 1 / (l^2 + 2 s), c0 = -1/2 sum log1p(2 s / l^2); with GRAD a third constant per
// dimension ahead of c0, 2 s r (formed in float64: 1 - l^2 r would cancel at small s).  A bad row (a negative, NaN or
// infinite variance) gets zeros and c0 = -inf; badpart[blockIdx.x] = the workgroup's count of bad rows.
template <typename T, int D, bool GRAD>
__global__ __launch_bounds__(256)
void k_psi2_rows(const T* __restrict__ mu, const T* __restrict__ s, int n, const double* __restrict__ ell, T* __restrict__ rc,
                 double* __restrict__ badpart)
{
    constexpr int RS = (GRAD ? 3 : 2) * D + 1;
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
            if constexpr (GRAD) o[2 * D + e] = (T)(2.0 * sv / (l2 + 2.0 * sv));
            lg += log1p(2.0 * sv / l2);
        }
        o[RS - 1] = (T)(-0.5 * lg);
        if (!ok) {
            bad = 1.0;
#pragma unroll
            for (int k = 0; k < RS - 1; ++k) o[k] = (T)0;
            o[RS - 1] = -(T)INFINITY;
        }
#pragma unroll
        for (int k = 0; k < RS; ++k) rc[(int64_t)i * RS + k] = o[k];
    }
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) badpart[blockIdx.x] = bad;
}

}  // namespace

}  // namespace cimrgp
