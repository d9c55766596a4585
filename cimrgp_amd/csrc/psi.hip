// The psi statistics of the RBF covariance under Gaussian inputs: the calls of include/cimrgp_psi.h.
//   psi1   k_psi1          a wave per row (wave_row, reduce.hpp): the row's d + 1 constants once per lane, then lane l
//                          writes columns l, l + 64, ..: one exponential per entry
//   psi2   k_psi2_rows     a thread per row: the row's 2 d + 1 constants (mu_e, 1 / (l_e^2 + 2 s_e), -1/2 sum log1p(2 s_e /
//                          l_e^2)) in float64, rounded once; a bad row gets (0, 0, -inf) and is counted per workgroup
//          k_psi2_tiles    one 64 x 64 tile of pairs (j, k) and one slice of the rows per workgroup; the partial tile
//                          goes to scratch
//          k_psi2_reduce   adds the slices' partials in slice order, multiplies by sf2^2 exp(-sum (z_j - z_k)^2 / 4 l^2),
//                          writes lower(C); its last workgroup adds the per-workgroup counts of bad rows
//
// k_psi2_tiles.  The sum over the rows has one exponential per (row, pair) and nothing the matrix cores could take: the
// denominators l^2 + 2 s differ from row to row.  Thread (ty, tx) of the 16 x 16 owns the pairs (ty + 16 a, tx + 16 b),
// a, b < 4: z_j / 2 and z_k / 2 of its 4 + 4 points stay in registers (halving is exact), (z_j + z_k) / 2 is never held per
// pair: the exponent is c0 - sum_e ((mu_e - z_je / 2) - z_ke / 2)^2 r_e, the direct form -- the expanded form
// 1/2 (mu - z_j)^2 + 1/2 (mu - z_k)^2 - 1/4 (z_j - z_k)^2 cancels when z_j and z_k are far apart with mu between them.
// The rows' constants are the same for every thread: 64 rows of them at a time are copied to LDS and read from there at
// one address per instruction (a broadcast).  The 16 x 16 blocks of a tile that hold no wanted pair -- above the
// diagonal of a diagonal tile, beyond row or column m -- are skipped: the condition is uniform over the workgroup.  A
// tile off the diagonal and inside m (FULL) has no such test, so its 16 exponentials per row interleave freely.
// Every partial sum is taken in one fixed order: a thread adds its slice's rows in row order, k_psi2_reduce the slices
// in slice order.
#include "psi_common.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

constexpr int PT = CIMRGP_PSI2_TILE;          // tile edge (pairs)
constexpr int PR = 4;                         // pairs per thread and side: 16 x 16 threads
constexpr int PCHUNK = 64;                    // rows whose constants are staged at a time
static_assert(PT == 16 * PR, "a 16 x 16 workgroup of PR x PR register tiles covers the tile");

// S(n, m) and the slice length: the rule of include/cimrgp_psi.h, a function of n and m alone (psi_common.hpp).
static inline int64_t psi2_tiles_1d(int64_t m) { return psi_tiles_1d(m, PT); }
static inline int64_t psi2_tiles(int64_t m) { return psi_tiles(m, PT); }
static inline int64_t psi2_slice_len(int64_t n, int64_t m) { return psi_slice_len(n, psi2_tiles(m), CIMRGP_PSI2_TARGET_WGS); }
static inline int64_t psi2_slices(int64_t n, int64_t m) { return psi_slice_count(n, psi2_slice_len(n, m)); }

// the three parts of the scratch in bytes, each a multiple of 16: the counts, the rows' constants, the partial tiles
static inline int64_t psi2_rows_bytes(int dtype, int64_t n, int d) { return round16(n * (2 * d + 1) * (int64_t)elem_bytes(dtype)); }
static inline int64_t psi2_part_bytes(int dtype, int64_t n, int64_t m)
{
    return psi2_slices(n, m) * psi2_tiles(m) * (PT * PT) * (int64_t)elem_bytes(dtype);
}

// ----------------------------------------------------------------------- psi1 ----
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi1(const T* __restrict__ mu, const T* __restrict__ s, const T* __restrict__ z, int n, int m,
            const double* __restrict__ ell, T sf2, T* __restrict__ out, int64_t ldo)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    T mv[D], hr[D];                              // mu_e and 1 / (2 (l_e^2 + s_e))
    double lg = 0.0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const double sv = (double)s[(int64_t)row * D + e], l2 = ell[e] * ell[e];
        mv[e] = mu[(int64_t)row * D + e];
        hr[e] = (T)(0.5 / (l2 + sv));
        lg += log1p(sv / l2);
    }
    const T c0 = (T)(-0.5 * lg);
    T* orow = out + (int64_t)row * ldo;
    for (int j = lane; j < m; j += 64) {
        T ex = c0;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const T df = mv[e] - z[(int64_t)j * D + e];
            ex = fma(-(df * df), hr[e], ex);
        }
        orow[j] = sf2 * t_exp(ex);
    }
}

// ----------------------------------------------------------------------- psi2 ----
// (k_psi2_rows, the pass over the rows: psi_common.hpp)
template <typename T, int D, bool FULL>
static __device__ __forceinline__ void psi2_tile(T* __restrict__ lds, const T* __restrict__ z, int m, const T* __restrict__ rc, int ti,
                                                 int tj, int k0, int k1, T* __restrict__ ctile)
{
    constexpr int RS = 2 * D + 1;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = ti * PT, j0 = tj * PT;
    const bool diag = ti == tj;
    T hzi[PR][D], hzj[PR][D], acc[PR][PR];
#pragma unroll
    for (int a = 0; a < PR; ++a) {
        const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * a;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            hzi[a][e] = (FULL || gi < m) ? (T)0.5 * z[(int64_t)gi * D + e] : (T)0;
            hzj[a][e] = (FULL || gj < m) ? (T)0.5 * z[(int64_t)gj * D + e] : (T)0;
        }
#pragma unroll
        for (int b = 0; b < PR; ++b) acc[a][b] = (T)0;
    }
    for (int kb = k0; kb < k1; kb += PCHUNK) {
        const int rows = min(PCHUNK, k1 - kb);
        __syncthreads();                                          // the previous chunk has been read
        for (int idx = tid; idx < rows * RS; idx += 256) lds[idx] = rc[(int64_t)kb * RS + idx];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const T* c = lds + r * RS;
            const T c0 = c[2 * D];
#pragma unroll
            for (int a = 0; a < PR; ++a) {
                if (!FULL && i0 + 16 * a >= m) continue;
                T di[D];
#pragma unroll
                for (int e = 0; e < D; ++e) di[e] = c[e] - hzi[a][e];
#pragma unroll
                for (int b = 0; b < PR; ++b) {
                    if (!FULL && (j0 + 16 * b >= m || (diag && b > a))) continue;
                    T ex = c0;
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        const T dl = di[e] - hzj[b][e];
                        ex = fma(-(dl * dl), c[D + e], ex);
                    }
                    acc[a][b] += t_exp(ex);
                }
            }
        }
    }
    // the partial tile, 64 x 64 row-major (whole tiles: no bounds; a skipped block holds zeros)
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int b = 0; b < PR; ++b) ctile[(ty + 16 * a) * PT + tx + 16 * b] = acc[a][b];
}

// blockIdx.x = tile + tiles * slice
template <typename T, int D>
__global__ __launch_bounds__(256, 2)
void k_psi2_tiles(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, int tiles1d, int tiles, int slice_len,
                  T* __restrict__ cpart)
{
    __shared__ T lds[PCHUNK * (2 * D + 1)];
    const int slice = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - slice * tiles;
    int ti, tj;
    psi2_tile_of(tile, tiles1d, ti, tj);
    const int k0 = slice * slice_len, k1 = min(n, k0 + slice_len);
    T* ctile = cpart + ((int64_t)slice * tiles + tile) * (PT * PT);
    if (ti != tj && (ti + 1) * PT <= m) psi2_tile<T, D, true>(lds, z, m, rc, ti, tj, k0, k1, ctile);
    else                                psi2_tile<T, D, false>(lds, z, m, rc, ti, tj, k0, k1, ctile);
}

// blockIdx.x < tiles * 16: 256 elements of one tile (four rows of it); the last workgroup: the count of bad rows, the
// per-workgroup counts added by thread t = i mod 256, then pairwise in LDS (lds_tree).  Only k <= j of C is written.
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2_reduce(const T* __restrict__ cpart, const T* __restrict__ z, int m, const double* __restrict__ ell, int tiles1d, int tiles,
                   int slices, T sf4, T* __restrict__ C, int64_t ldc, const double* __restrict__ badpart, int nbad,
                   double* __restrict__ bad)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == tiles * 16) {
        double b = 0.0;
        for (int i = tid; i < nbad; i += 256) b += badpart[i];
        red[tid] = b;
        lds_tree<256>(red, tid);
        if (tid == 0) bad[0] = red[0];
        return;
    }
    const int tile = (int)blockIdx.x >> 4, part = (int)blockIdx.x & 15;
    int ti, tj;
    psi2_tile_of(tile, tiles1d, ti, tj);
    const int el = part * 256 + tid;
    const int i = ti * PT + (el >> 6), j = tj * PT + (el & 63);
    if (i >= m || j > i) return;
    const T* p = cpart + (int64_t)tile * (PT * PT) + el;
    T sum = p[0];
    for (int sl = 1; sl < slices; ++sl) sum += p[(int64_t)sl * tiles * (PT * PT)];
    T zx = (T)0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const T df = z[(int64_t)i * D + e] - z[(int64_t)j * D + e];
        zx = fma(df * df, (T)(0.25 / (ell[e] * ell[e])), zx);
    }
    C[(int64_t)i * ldc + j] = sf4 * t_exp(-zx) * sum;
}

template <typename T>
static int psi1_run(const T* mu, const T* s, const T* z, int64_t n, int64_t m, int d, const double* ell, double sf2, T* out, int64_t ldo,
                    hipStream_t st, const char* fn)
{
    with_dim_exact(d, [&](auto dd) {
        hipLaunchKernelGGL((k_psi1<T, decltype(dd)::value>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, mu, s, z, (int)n, (int)m, ell,
                           (T)sf2, out, ldo);
    });
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
static int psi2_run(int dtype, const T* mu, const T* s, const T* z, int64_t n, int64_t m, int d, const double* ell, double sf2, T* c,
                    int64_t ldc, char* scratch, double* bad, hipStream_t st, const char* fn)
{
    const int64_t t1 = psi2_tiles_1d(m), tiles = psi2_tiles(m), len = psi2_slice_len(n, m), slices = psi2_slices(n, m);
    const int64_t nb = psi2_count_blocks(n);
    double* badpart = reinterpret_cast<double*>(scratch);
    T* rc = reinterpret_cast<T*>(scratch + psi2_count_bytes(n));
    T* cpart = reinterpret_cast<T*>(scratch + psi2_count_bytes(n) + psi2_rows_bytes(dtype, n, d));
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi2_rows<T, D>), dim3((unsigned)nb), dim3(256), 0, st, mu, s, (int)n, ell, rc, badpart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2_tiles<T, D>), dim3((unsigned)(tiles * slices)), dim3(256), 0, st, z, (int)m, (const T*)rc, (int)n,
                           (int)t1, (int)tiles, (int)len, cpart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2_reduce<T, D>), dim3((unsigned)(tiles * 16 + 1)), dim3(256), 0, st, (const T*)cpart, z, (int)m, ell,
                           (int)t1, (int)tiles, (int)slices, (T)(sf2 * sf2), c, ldc, (const double*)badpart, (int)nb, bad);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_psi1(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d, const double* ell_dev,
                double sf2, void* out_dev, int64_t ldo, void* stream)
{
    const char* fn = "cimrgp_psi1";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(mu_dev && s_dev && z_dev && ell_dev && out_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && n < (1ll << 31), fn, "n must be in [0, 2^31)");
    CIMRGP_REQUIRE(m >= 1 && m < (1ll << 31), fn, "m must be in [1, 2^31)");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(sf2 > 0.0, fn, "sf2 must be positive");
    CIMRGP_REQUIRE(ldo >= m, fn, "leading dimension too small");
    if (n == 0) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return psi1_run<T>((const T*)mu_dev, (const T*)s_dev, (const T*)z_dev, n, m, d, ell_dev, sf2, (T*)out_dev, ldo, stream_of(stream),
                           fn);
    });
}

int cimrgp_psi2_slices(int64_t n, int64_t m)
{
    return psi2_sizes_ok(n, m) ? (int)psi2_slices(n, m) : 0;
}

size_t cimrgp_psi2_scratch_bytes(int dtype, int64_t n, int64_t m, int d)
{
    if (!dtype_known(dtype) || !psi2_sizes_ok(n, m) || d < 1 || d > MAXD) return 0;
    return (size_t)(psi2_count_bytes(n) + psi2_rows_bytes(dtype, n, d) + psi2_part_bytes(dtype, n, m));
}

int cimrgp_psi2(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d, const double* ell_dev,
                double sf2, void* c_dev, int64_t ldc, void* scratch_dev, size_t scratch_bytes, double* bad_dev, void* stream)
{
    const char* fn = "cimrgp_psi2";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(mu_dev && s_dev && z_dev && ell_dev && c_dev && scratch_dev && bad_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n <= CIMRGP_PSI2_MAX_N, fn, "n must be in [1, 16777216]");
    CIMRGP_REQUIRE(m >= 1 && m <= CIMRGP_PSI2_MAX_M, fn, "m must be in [1, 16384]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(sf2 > 0.0, fn, "sf2 must be positive");
    CIMRGP_REQUIRE(ldc >= m, fn, "leading dimension too small");
    CIMRGP_REQUIRE(aligned16(scratch_dev), fn, "scratch must be 16-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_psi2_scratch_bytes(dtype, n, m, d), fn, "scratch too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return psi2_run<T>(dtype, (const T*)mu_dev, (const T*)s_dev, (const T*)z_dev, n, m, d, ell_dev, sf2, (T*)c_dev, ldc,
                           (char*)scratch_dev, bad_dev, stream_of(stream), fn);
    });
}

}  // extern "C"
