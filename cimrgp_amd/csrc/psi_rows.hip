// One row's own Psi2 contracted with weights: the calls of include/cimrgp_psi_rows.h.
//   psi2_rows_quad  k_psi2_rows     the pass over the rows (psi_common.hpp): the 2 d + 1 constants, the bad rows
//                   k_psi2rq_pass   a thread per row (psi2_own_row), 256 rows per workgroup, over one group of the 64 x 64
//                                   tiles of the lower triangle (the header's rule: the groups depend on m alone); the
//                                   row's 1 + q subtotals of the group go to scratch
//                   k_psi2rq_reduce adds a row's subtotals in group order (psi_ordered_sum), writes tr and quad; its last
//                                   workgroup adds the per-workgroup counts of bad rows (psi2_count_bad)
//
// k_psi2rq_pass.  Per tile the workgroup stages z / 2 of the tile's 64 + 64 points (psi2_stage_points) and their rows of
// a (columns >= q as zeros), and, RW rows of the tile at a time, the two weights of a pair:
// e_jk = w sf2^2 exp(-delta_jk) and e_jk c_jk (w = 1 on the diagonal, 2 off it; 0 outside k <= j < m).  Every thread reads
// the same LDS word in the same instruction (a broadcast).  Per (row, pair): the exponent
// (psi2_exponent), ONE exponential p0, tr += (e c)_jk p0, and with p = e_jk p0 one multiply-add per output into
// inner_c = sum_{k <= j} a_kc p; after the k of one j, quad_c += a_jc inner_c.
// A bad row has c0 = -infinity: p0 is exactly 0 and so is every sum.
// The order of every sum is fixed by (m, d, q): tiles in tile order within the group, j then k ascending within a tile.
#include "psi_common.hpp"

namespace cimrgp {

namespace {

constexpr int RW = 32;                        // rows of a tile whose weights are staged at a time
static_assert(PSI_TILE % RW == 0 && (RW * PSI_TILE) % 256 == 0, "the weights are staged by whole workgroups");

// ---- the geometry: the header's grouping, a function of m alone ----
static inline int64_t psirq_group_tiles(int64_t m)
{
    const int64_t tiles = psi_tiles(m, PSI_TILE);
    return (tiles + CIMRGP_PSI_ROWS_GROUPS - 1) / CIMRGP_PSI_ROWS_GROUPS;
}
static inline int64_t psirq_groups(int64_t m)
{
    const int64_t g = psirq_group_tiles(m);
    return (psi_tiles(m, PSI_TILE) + g - 1) / g;
}
// cimrgp_psi2_rows_quad's scratch: the counts of bad rows at 0, the rows' constants, then the (group, row) subtotals
struct PsiRowsScratch { int64_t rc, part, total; };
static inline PsiRowsScratch psirq_scratch(int dtype, int64_t n, int64_t m, int d, int q)
{
    const int64_t rc = psi2_count_bytes(n), part = rc + psi2_rows_bytes(dtype, n, d);
    return {rc, part, part + round16(psirq_groups(m) * n * (1 + q) * (int64_t)elem_bytes(dtype))};
}
static inline bool psirq_sizes_ok(int64_t n, int64_t m, int d, int q)
{
    return psi2_sizes_ok(n, m) && d >= 1 && d <= MAXD && q >= 1 && q <= MAXQ;
}

// blockIdx.x = row block + rowblocks * group.  part[(group n + i) (1 + q) + ..] = the group's (tr_i, quad_i0 .. quad_i,q-1).
// Q >= q: the compile-time number of outputs (with_q_rounded); columns >= q of a are staged as zeros and never written.
template <typename T, int D, int Q>
__global__ __launch_bounds__(256)
void k_psi2rq_pass(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, const double* __restrict__ ell, T sf4,
                   const T* __restrict__ cm, int64_t ldc, const T* __restrict__ am, int64_t lda, int q, int rowblocks, int tiles1d,
                   int tiles, int group_tiles, T* __restrict__ part)
{
    constexpr int RS = 2 * D + 1;
    __shared__ T we[RW * PSI_TILE], wc[RW * PSI_TILE];
    __shared__ T hzi[PSI_TILE * D], hzj[PSI_TILE * D], ai[PSI_TILE * Q], aj[PSI_TILE * Q];
    const int tid = threadIdx.x;
    const int group = (int)blockIdx.x / rowblocks, rb = (int)blockIdx.x - group * rowblocks;
    const int i = rb * 256 + tid;
    const bool live = i < n;
    T mv[D], rv[D], il2[D], qd[Q], tr = (T)0;
    const T c0 = psi2_own_row<T, D, RS>(rc, i, live, ell, mv, rv, il2);
#pragma unroll
    for (int c = 0; c < Q; ++c) qd[c] = (T)0;
    const int t0 = group * group_tiles, t1 = min(tiles, t0 + group_tiles);
    for (int tile = t0; tile < t1; ++tile) {
        int ti, tj;
        psi2_tile_of(tile, tiles1d, ti, tj);
        const int i0 = ti * PSI_TILE, j0 = tj * PSI_TILE;
        __syncthreads();                                          // the previous tile has been read
        psi2_stage_points<T, D>(z, m, i0, j0, hzi, hzj, tid);
        for (int idx = tid; idx < PSI_TILE * Q; idx += 256) {
            const int gi = i0 + idx / Q, gj = j0 + idx / Q, c = idx % Q;
            ai[idx] = (gi < m && c < q) ? am[(int64_t)gi * lda + c] : (T)0;
            aj[idx] = (gj < m && c < q) ? am[(int64_t)gj * lda + c] : (T)0;
            if (idx + 256 >= PSI_TILE * Q) lds_settle(aj + idx);
        }
        const int na = min(PSI_TILE, m - i0);
        for (int a0 = 0; a0 < na; a0 += RW) {
            __syncthreads();                                      // z / 2 and a are in place; the previous weights have been read
            // the weights of rows a0 .. a0 + RW - 1 of the tile: 0 outside k <= j < m, where c is not read
#pragma unroll 4
            for (int u = 0; u < RW * PSI_TILE / 256; ++u) {
                const int el = tid + 256 * u, a = a0 + (el >> 6), b = el & 63;
                const int gj = i0 + a, gk = j0 + b;
                T ve = (T)0, vc = (T)0;
                if (gj < m && gk <= gj) {
                    T zx = (T)0;
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        const T df = hzi[a * D + e] - hzj[b * D + e];
                        zx = fma(df * df, il2[e], zx);
                    }
                    ve = (gj == gk ? (T)1 : (T)2) * (sf4 * t_exp(-zx));
                    vc = ve * cm[(int64_t)gj * ldc + gk];
                }
                we[el] = ve;
                wc[el] = vc;
            }
            lds_settle(wc + tid + 256 * (RW * PSI_TILE / 256 - 1));
            __syncthreads();
            if (live) {
                const int a1 = min(na, a0 + RW);
                for (int a = a0; a < a1; ++a) {
                    T di[D], inner[Q];
#pragma unroll
                    for (int e = 0; e < D; ++e) di[e] = mv[e] - hzi[a * D + e];
#pragma unroll
                    for (int c = 0; c < Q; ++c) inner[c] = (T)0;
                    const int nb = ti == tj ? a + 1 : PSI_TILE;
                    const T* wer = we + (a - a0) * PSI_TILE;
                    const T* wcr = wc + (a - a0) * PSI_TILE;
#pragma unroll 2
                    for (int b = 0; b < nb; ++b) {
                        const T p0 = t_exp(psi2_exponent<T, D, false>(c0, di, hzj + b * D, rv));
                        tr = fma(wcr[b], p0, tr);
                        const T p = wer[b] * p0;
#pragma unroll
                        for (int c = 0; c < Q; ++c) inner[c] = fma(aj[b * Q + c], p, inner[c]);
                    }
#pragma unroll
                    for (int c = 0; c < Q; ++c) qd[c] = fma(ai[a * Q + c], inner[c], qd[c]);
                }
            }
        }
    }
    if (live) {
        T* o = part + ((int64_t)group * n + i) * (1 + q);
        o[0] = tr;
#pragma unroll
        for (int c = 0; c < Q; ++c)
            if (c < q) o[1 + c] = qd[c];
    }
}

// blockIdx.x < ceil(n (1 + q) / 256): one of a row's 1 + q sums per thread, the groups in group order; the last workgroup:
// the count of bad rows
template <typename T>
__global__ __launch_bounds__(256)
void k_psi2rq_reduce(const T* __restrict__ part, int n, int q, int groups, T* __restrict__ tr, T* __restrict__ quad, int64_t ldq,
                     const double* __restrict__ badpart, int nbad, double* __restrict__ bad)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        psi2_count_bad(badpart, nbad, red, tid, bad);
        return;
    }
    const int64_t idx = (int64_t)blockIdx.x * 256 + tid, total = (int64_t)n * (1 + q);
    if (idx >= total) return;
    const int64_t i = idx / (1 + q);
    const int c = (int)(idx - i * (1 + q));
    const T acc = psi_ordered_sum(part + idx, groups, total);
    if (c == 0) tr[i] = acc;
    else        quad[i * ldq + (c - 1)] = acc;
}

template <typename T>
static int psirq_run(int dtype, const T* mu, const T* s, const T* z, int64_t n, int64_t m, int d, const double* ell, double sf2, const T* cm,
                     int64_t ldc, const T* am, int64_t lda, int q, T* tr, T* quad, int64_t ldq, char* scratch, double* bad, hipStream_t st,
                     const char* fn)
{
    const int64_t nb = psi2_count_blocks(n), t1 = psi_tiles_1d(m, PSI_TILE), tiles = psi_tiles(m, PSI_TILE);
    const int64_t gt = psirq_group_tiles(m), groups = psirq_groups(m);
    double* badpart = reinterpret_cast<double*>(scratch);
    const PsiRowsScratch lay = psirq_scratch(dtype, n, m, d, q);
    T* rc = reinterpret_cast<T*>(scratch + lay.rc);
    T* part = reinterpret_cast<T*>(scratch + lay.part);
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi2_rows<T, D, false>), dim3((unsigned)nb), dim3(256), 0, st, mu, s, (int)n, ell, rc, badpart);
        CIMRGP_LAUNCH_CHECK(fn);
        with_q_rounded(q, [&](auto qq) {
            hipLaunchKernelGGL((k_psi2rq_pass<T, D, decltype(qq)::value>), dim3((unsigned)(nb * groups)), dim3(256), 0, st, z, (int)m,
                               (const T*)rc, (int)n, ell, (T)(sf2 * sf2), cm, ldc, am, lda, q, (int)nb, (int)t1, (int)tiles, (int)gt, part);
        });
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2rq_reduce<T>), dim3((unsigned)((n * (1 + q) + 255) / 256 + 1)), dim3(256), 0, st, (const T*)part, (int)n, q,
                           (int)groups, tr, quad, ldq, (const double*)badpart, (int)nb, bad);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

size_t cimrgp_psi2_rows_quad_scratch_bytes(int dtype, int64_t n, int64_t m, int d, int q)
{
    if (!dtype_known(dtype) || !psirq_sizes_ok(n, m, d, q)) return 0;
    return (size_t)psirq_scratch(dtype, n, m, d, q).total;
}

int cimrgp_psi2_rows_quad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d,
                          const double* ell_dev, double sf2, const void* c_dev, int64_t ldc, const void* a_dev, int64_t lda, int q,
                          void* tr_dev, void* quad_dev, int64_t ldq, void* scratch_dev, size_t scratch_bytes, double* bad_dev, void* stream)
{
    const char* fn = "cimrgp_psi2_rows_quad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(mu_dev && s_dev && z_dev && ell_dev && c_dev && a_dev && tr_dev && quad_dev && scratch_dev && bad_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n <= CIMRGP_PSI2_MAX_N, fn, "n must be in [1, 16777216]");
    CIMRGP_REQUIRE(m >= 1 && m <= CIMRGP_PSI2_MAX_M, fn, "m must be in [1, 16384]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "the number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(sf2 > 0.0, fn, "sf2 must be positive");
    CIMRGP_REQUIRE(ldc >= m && lda >= q && ldq >= q, fn, "leading dimension too small");
    CIMRGP_REQUIRE(aligned16(scratch_dev), fn, "scratch must be 16-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_psi2_rows_quad_scratch_bytes(dtype, n, m, d, q), fn, "scratch too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return psirq_run<T>(dtype, (const T*)mu_dev, (const T*)s_dev, (const T*)z_dev, n, m, d, ell_dev, sf2, (const T*)c_dev, ldc,
                            (const T*)a_dev, lda, q, (T*)tr_dev, (T*)quad_dev, ldq, (char*)scratch_dev, bad_dev, stream_of(stream), fn);
    });
}

}  // extern "C"
