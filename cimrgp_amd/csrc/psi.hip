// The psi statistics of the RBF covariance under Gaussian inputs: the calls of include/cimrgp_psi.h.
//   psi1   k_psi1          a wave per row (wave_row, reduce.hpp): the row's d + 1 constants once per lane
//                          (psi1_row_consts), then lane l writes columns l, l + 64, ..: one exponential per entry
//   psi2   k_psi2_rows     the pass over the rows (psi_common.hpp): a row's 2 d + 1 constants, the bad rows counted
//          k_psi2_tiles    one 64 x 64 tile of pairs (j, k) and one slice of the rows per workgroup; the partial tile
//                          goes to scratch
//          k_psi2_reduce   adds the slices' partials in slice order (psi_ordered_sum), multiplies by
//                          sf2^2 exp(-sum (z_j - z_k)^2 / 4 l^2), writes lower(C); its last workgroup adds the
//                          per-workgroup counts of bad rows (psi2_count_bad)
//
// k_psi2_tiles.  The sum over the rows has one exponential per (row, pair) and nothing the matrix cores could take: the
// denominators l^2 + 2 s differ from row to row.  Thread (ty, tx) of the 16 x 16 owns the pairs (ty + 16 a, tx + 16 b),
// a, b < 4: z / 2 of its 4 + 4 points stays in registers (psi2_pair_points) for the exponent in its direct form
// (psi2_exponent).  The rows' constants are the same for every thread: 64 rows of them at a time are copied to LDS
// (psi2_stage_chunk) and read from there at one address per instruction (a broadcast).  The 16 x 16 blocks of a tile
// that hold no wanted pair -- above the diagonal of a diagonal tile, beyond row or column m -- are skipped: the
// condition is uniform over the workgroup.  A tile off the diagonal and inside m (FULL) has no such test, so its 16
// exponentials per row interleave freely.  Every partial sum is taken in one fixed order: a thread adds its slice's
// rows in row order, k_psi2_reduce the slices in slice order.
#include "psi_common.hpp"

namespace cimrgp {

namespace {

constexpr int PR = 4;                         // pairs per thread and side: 16 x 16 threads
static_assert(PSI_TILE == 16 * PR, "a 16 x 16 workgroup of PR x PR register tiles covers the tile");

// S(n, m) and the slice length: the rule of include/cimrgp_psi.h, a function of n and m alone (psi_common.hpp).
static inline int64_t psi2_slice_len(int64_t n, int64_t m) { return psi_slice_len(n, psi_tiles(m, PSI_TILE), CIMRGP_PSI2_TARGET_WGS); }
static inline int64_t psi2_slices(int64_t n, int64_t m) { return psi_slice_count(n, psi2_slice_len(n, m)); }

// cimrgp_psi2's scratch: the counts of bad rows at 0, then the rows' constants, then the partial tiles
struct Psi2Scratch { int64_t rc, cpart, total; };
static inline Psi2Scratch psi2_scratch(int dtype, int64_t n, int64_t m, int d)
{
    const int64_t rc = psi2_count_bytes(n), cpart = rc + psi2_rows_bytes(dtype, n, d);
    return {rc, cpart, cpart + psi2_slices(n, m) * psi_tiles(m, PSI_TILE) * (PSI_TILE * PSI_TILE) * (int64_t)elem_bytes(dtype)};
}

// ----------------------------------------------------------------------- psi1 ----
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi1(const T* __restrict__ mu, const T* __restrict__ s, const T* __restrict__ z, int n, int m,
            const double* __restrict__ ell, T sf2, T* __restrict__ out, int64_t ldo)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    T mv[D], hr[D];
    const T c0 = psi1_row_consts<T, D>(mu, s, row, ell, mv, hr);
    T* orow = out + (int64_t)row * ldo;
    for (int j = lane; j < m; j += 64) orow[j] = sf2 * t_exp(psi1_exponent<T, D>(c0, mv, z + (int64_t)j * D, hr));
}

// ----------------------------------------------------------------------- psi2 ----
// One tile (ti, tj) and the rows k0 .. k1 - 1: the partial tile, 64 x 64 row-major (whole tiles: no bounds; a skipped
// block holds zeros)
template <typename T, int D, bool FULL>
static __device__ __forceinline__ void psi2_tile(T* __restrict__ lds, const T* __restrict__ z, int m, const T* __restrict__ rc, int ti,
                                                 int tj, int k0, int k1, T* __restrict__ ctile)
{
    constexpr int RS = 2 * D + 1;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = ti * PSI_TILE, j0 = tj * PSI_TILE;
    const bool diag = ti == tj;
    T hzi[PR][D], hzj[PR][D], acc[PR][PR];
    psi2_pair_points<T, D, PR, FULL>(z, m, i0, j0, ty, tx, hzi, hzj);
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int b = 0; b < PR; ++b) acc[a][b] = (T)0;
    for (int kb = k0; kb < k1; kb += PSI_CHUNK) {
        const int rows = min(PSI_CHUNK, k1 - kb);
        psi2_stage_chunk(lds, rc + (int64_t)kb * RS, rows * RS, tid);
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
                    acc[a][b] += t_exp(psi2_exponent<T, D, false>(c0, di, hzj[b], c + D));
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int b = 0; b < PR; ++b) ctile[(ty + 16 * a) * PSI_TILE + tx + 16 * b] = acc[a][b];
}

// blockIdx.x = tile + tiles * slice
template <typename T, int D>
__global__ __launch_bounds__(256, 2)
void k_psi2_tiles(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, int tiles1d, int tiles, int slice_len,
                  T* __restrict__ cpart)
{
    __shared__ T lds[PSI_CHUNK * (2 * D + 1)];
    const int slice = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - slice * tiles;
    int ti, tj;
    psi2_tile_of(tile, tiles1d, ti, tj);
    const int k0 = slice * slice_len, k1 = min(n, k0 + slice_len);
    T* ctile = cpart + ((int64_t)slice * tiles + tile) * (PSI_TILE * PSI_TILE);
    if (ti != tj && (ti + 1) * PSI_TILE <= m) psi2_tile<T, D, true>(lds, z, m, rc, ti, tj, k0, k1, ctile);
    else                                psi2_tile<T, D, false>(lds, z, m, rc, ti, tj, k0, k1, ctile);
}

// blockIdx.x < tiles * 16: 256 elements of one tile (four rows of it); the last workgroup: the count of bad rows.  Only
// k <= j of C is written.
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2_reduce(const T* __restrict__ cpart, const T* __restrict__ z, int m, const double* __restrict__ ell, int tiles1d, int tiles,
                   int slices, T sf4, T* __restrict__ C, int64_t ldc, const double* __restrict__ badpart, int nbad,
                   double* __restrict__ bad)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == tiles * 16) {
        psi2_count_bad(badpart, nbad, red, tid, bad);
        return;
    }
    const int tile = (int)blockIdx.x >> 4, part = (int)blockIdx.x & 15;
    int ti, tj;
    psi2_tile_of(tile, tiles1d, ti, tj);
    const int el = part * 256 + tid;
    const int i = ti * PSI_TILE + (el >> 6), j = tj * PSI_TILE + (el & 63);
    if (i >= m || j > i) return;
    const T sum = psi_ordered_sum(cpart + (int64_t)tile * (PSI_TILE * PSI_TILE) + el, slices, (int64_t)tiles * (PSI_TILE * PSI_TILE));
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
    const int64_t t1 = psi_tiles_1d(m, PSI_TILE), tiles = psi_tiles(m, PSI_TILE), len = psi2_slice_len(n, m), slices = psi2_slices(n, m);
    const int64_t nb = psi2_count_blocks(n);
    const Psi2Scratch lay = psi2_scratch(dtype, n, m, d);
    double* badpart = reinterpret_cast<double*>(scratch);
    T* rc = reinterpret_cast<T*>(scratch + lay.rc);
    T* cpart = reinterpret_cast<T*>(scratch + lay.cpart);
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi2_rows<T, D, false>), dim3((unsigned)nb), dim3(256), 0, st, mu, s, (int)n, ell, rc, badpart);
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
    return (size_t)psi2_scratch(dtype, n, m, d).total;
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
