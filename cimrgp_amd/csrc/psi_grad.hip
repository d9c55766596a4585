// The derivatives of the psi statistics contracted with a weight matrix: the calls of include/cimrgp_psi_grad.h.
//   psi1_grad  k_psi1g_rows        a wave per row (wave_row): Psi1 from psi1_row_consts and psi1_exponent, lane l takes
//                                  columns l, l + 64, ..; wave_sum of the row's 2 d + 1 sums, lane 0 writes dmu and ds
//              k_psi1g_cols        a thread per column, one wave per workgroup, over one slice of the rows: a chunk's
//                                  row constants are formed by the wave (psi1_row_consts) and read back from LDS at one
//                                  address per instruction; partial dz per (slice, column), partial sums per (slice,
//                                  column block)
//              k_psi1g_reduce      adds the slices in slice order (psi_ordered_sum); its last workgroup adds the sums
//   psi2_grad  k_psi2_rows         the pass over the rows (psi_common.hpp) with its third constant per dimension, 2 s r
//              k_psi2g_rowpass     a thread per row (psi2_own_row), 256 rows per workgroup, over share p of the 64 x 64
//                                  tiles of the lower triangle (tiles p, p + P, ..): z / 2 of the tile's points
//                                  (psi2_stage_points) and the pairs' weights in LDS, read at one address per instruction
//              k_psi2g_rowreduce   adds the P shares in order (psi_ordered_sum): dmu, ds
//              k_psi2g_pairs       k_psi2_tiles' walk (psi.hip) over a tile of edge 16 PR, PR = 4 (d <= 2) or 2, on the same
//                                  pieces (psi2_pair_points, psi2_stage_chunk, psi2_exponent): per thread the sums of
//                                  q = dl r for its PR + PR points, of the log-l terms, and of the exponentials per pair
//                                  (the delta parts need Psi2_jk); then the 16 threads of a thread row / column are added
//                                  through LDS in thread order and the d + 1 sums by block_sum
//              k_psi2g_pairreduce  dz_j: slices in slice order, within a slice the tiles that hold point j in tile order;
//                                  its last workgroup adds the sums and the counts of bad rows (psi2_count_bad)
// Every hand-over through LDS is: stores, lds_settle on the last word stored, barrier (common.hpp).
// Every partial sum is taken in one fixed order that depends on (n, m, d) alone.
#include "psi_common.hpp"

namespace cimrgp {

namespace {

template <int D> struct PairGeom {
    static constexpr int PR = D <= 2 ? 4 : 2;                     // pairs per thread and side
    static constexpr int TG = 16 * PR;                            // tile edge: 16 x 16 threads
    static_assert(TG == CIMRGP_PSI_GRAD_PAIR_EDGE(D), "the header's tile edge");
};

// ---- the geometry, functions of (n, m, d) alone ----
static inline int64_t psi1g_colblocks(int64_t m) { return (m + 63) / 64; }
static inline int64_t psi1g_slice_len(int64_t n, int64_t m) { return psi_slice_len(n, psi1g_colblocks(m), CIMRGP_PSI2_TARGET_WGS); }
static inline int64_t psi2g_shares(int64_t n, int64_t m)
{
    int64_t p = CIMRGP_PSI_GRAD_ROW_WGS / psi2_count_blocks(n);
    const int64_t tiles = psi_tiles(m, PSI_TILE);
    if (p > tiles) p = tiles;
    return p < 1 ? 1 : p;
}
static inline int64_t psi2g_edge(int d) { return CIMRGP_PSI_GRAD_PAIR_EDGE(d); }
static inline int64_t psi2g_slice_len(int64_t n, int64_t m, int d) { return psi_slice_len(n, psi_tiles(m, psi2g_edge(d)), CIMRGP_PSI2_TARGET_WGS); }

// cimrgp_psi1_grad's scratch, each part a multiple of 16 bytes: the partial dz per (slice, column) at 0, then the partial
// sums per (slice, column block) in float64
struct Psi1GradScratch { int64_t spart, total; };
static inline Psi1GradScratch psi1g_scratch(int dtype, int64_t n, int64_t m, int d)
{
    const int64_t slices = psi_slice_count(n, psi1g_slice_len(n, m));
    const int64_t spart = round16(slices * m * d * (int64_t)elem_bytes(dtype));
    return {spart, spart + round16(slices * psi1g_colblocks(m) * (d + 1) * 8)};
}

// cimrgp_psi2_grad's scratch, each part a multiple of 16 bytes: the counts of bad rows at 0, the rows' constants, the
// shares' (dmu, ds), then per (slice, pair tile) the 2 edge d partial sums of dz and the d + 1 partial sums in float64
struct Psi2GradScratch { int64_t rc, rpart, zpart, spart, total; };
static inline Psi2GradScratch psi2g_scratch(int dtype, int64_t n, int64_t m, int d)
{
    const int64_t esz = (int64_t)elem_bytes(dtype);
    const int64_t units = psi_slice_count(n, psi2g_slice_len(n, m, d)) * psi_tiles(m, psi2g_edge(d));
    const int64_t rc = psi2_count_bytes(n), rpart = rc + psi2_rows_bytes(dtype, n, d, true);
    const int64_t zpart = rpart + round16(psi2g_shares(n, m) * n * 2 * d * esz);
    const int64_t spart = zpart + round16(units * 2 * psi2g_edge(d) * d * esz);
    return {rc, rpart, zpart, spart, spart + round16(units * (d + 1) * 8)};
}

// sums[c] = scale_c x the sum of part[i (D + 1) + c], i < count: thread t adds entries t, t + 256, .., then lds_tree
template <int D>
static __device__ __forceinline__ void add_sums(const double* __restrict__ part, int count, double first_scale, double* red, int tid,
                                                double* __restrict__ sums)
{
#pragma unroll
    for (int c = 0; c <= D; ++c) {
        double b = 0.0;
        for (int i = tid; i < count; i += 256) b += part[(int64_t)i * (D + 1) + c];
        red[c * 256 + tid] = b;
    }
    lds_tree<256, D + 1>(red, tid);
    if (tid <= D) sums[tid] = (tid == 0 ? first_scale : 1.0) * red[tid * 256];
}

// ------------------------------------------------------------------ psi1_grad ----
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi1g_rows(const T* __restrict__ mu, const T* __restrict__ s, const T* __restrict__ z, int n, int m, const double* __restrict__ ell,
                  T sf2, const T* __restrict__ g1, int64_t ldg, T* __restrict__ dmu, T* __restrict__ ds)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    T mv[D], hr[D];
    const T c0 = psi1_row_consts<T, D>(mu, s, row, ell, mv, hr);
    T am[D], aq[D], a0 = (T)0;                   // sum p q_e, sum p q_e^2, sum p: p = g1 Psi1, q_e = (mu_e - z_e) h_e
#pragma unroll
    for (int e = 0; e < D; ++e) am[e] = aq[e] = (T)0;
    const T* grow = g1 + (int64_t)row * ldg;
    for (int j = lane; j < m; j += 64) {
        T df[D];
        const T ex = psi1_exponent<T, D>(c0, mv, z + (int64_t)j * D, hr, df);
        const T p = grow[j] * (sf2 * t_exp(ex));
        a0 += p;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const T q = df[e] * ((T)2 * hr[e]), pq = p * q;
            am[e] += pq;
            aq[e] = fma(pq, q, aq[e]);
        }
    }
    wave_sum(am, aq, a0);
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < D; ++e) {
            dmu[(int64_t)row * D + e] = -am[e];
            ds[(int64_t)row * D + e] = (T)0.5 * (aq[e] - (T)2 * hr[e] * a0);
        }
    }
}

// blockIdx.x = column block + colblocks * slice; 64 threads.  lds: PSI_CHUNK rows of (mu_e, hr_e, 2 s_e hr_e, c0).
template <typename T, int D>
__global__ __launch_bounds__(64)
void k_psi1g_cols(const T* __restrict__ mu, const T* __restrict__ s, const T* __restrict__ z, int n, int m, const double* __restrict__ ell,
                  T sf2, const T* __restrict__ g1, int64_t ldg, int colblocks, int slice_len, T* __restrict__ zpart,
                  double* __restrict__ spart)
{
    constexpr int RS = 3 * D + 1;
    __shared__ T lds[PSI_CHUNK * RS];
    const int tid = threadIdx.x;
    const int slice = (int)blockIdx.x / colblocks, cb = (int)blockIdx.x - slice * colblocks;
    const int j = cb * 64 + tid;
    const bool live = j < m;
    const int k0 = slice * slice_len, k1 = min(n, k0 + slice_len);
    T zv[D], l2[D], az[D], al[D], a0 = (T)0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        zv[e] = live ? z[(int64_t)j * D + e] : (T)0;
        l2[e] = (T)(ell[e] * ell[e]);
        az[e] = al[e] = (T)0;
    }
    for (int kb = k0; kb < k1; kb += PSI_CHUNK) {
        const int rows = min(PSI_CHUNK, k1 - kb);
        __syncthreads();                                          // the previous chunk has been read
        if (tid < rows) {
            T* c = lds + tid * RS;
            c[3 * D] = psi1_row_consts<T, D, true>(mu, s, kb + tid, ell, c, c + D, c + 2 * D);
            lds_settle(c + 3 * D);
        }
        __syncthreads();
        if (live) {
            for (int r = 0; r < rows; ++r) {
                const T* c = lds + r * RS;
                T df[D];
                const T ex = psi1_exponent<T, D>(c[3 * D], c, zv, c + D, df);
                const T p = g1[(int64_t)(kb + r) * ldg + j] * (sf2 * t_exp(ex));
                a0 += p;
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    const T q = df[e] * ((T)2 * c[D + e]);
                    az[e] = fma(p, q, az[e]);
                    al[e] = fma(p, fma(l2[e] * q, q, c[2 * D + e]), al[e]);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < D; ++e) zpart[((int64_t)slice * m + j) * D + e] = az[e];
    }
    double v[D + 1];
    v[0] = (double)a0;
#pragma unroll
    for (int e = 0; e < D; ++e) v[1 + e] = (double)al[e];
    wave_sum(v);
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c <= D; ++c) spart[((int64_t)slice * colblocks + cb) * (D + 1) + c] = v[c];
    }
}

// blockIdx.x < ceil(m D / 256): one entry of dz per thread; the last workgroup: sums
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi1g_reduce(const T* __restrict__ zpart, const double* __restrict__ spart, int m, int slices, int nspart, T* __restrict__ dz,
                    double* __restrict__ sums)
{
    __shared__ double red[(D + 1) * 256];
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        add_sums<D>(spart, nspart, 1.0, red, tid, sums);
        return;
    }
    const int idx = (int)blockIdx.x * 256 + tid;
    if (idx >= m * D) return;
    dz[idx] = psi_ordered_sum(zpart + idx, slices, (int64_t)m * D);
}

// ------------------------------------------------------------------ psi2_grad ----
// (k_psi2_rows<T, D, true>, the pass over the rows: psi_common.hpp)
// blockIdx.x = row block + rowblocks * share.  rpart[(share n + i) 2 D + ..] = the share's (dmu_i, ds_i).
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_rowpass(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, const double* __restrict__ ell, T sf4,
                     const T* __restrict__ g2, int64_t ldg, int rowblocks, int shares, int tiles1d, int tiles, T* __restrict__ rpart)
{
    constexpr int RS = 3 * D + 1;
    __shared__ T w[PSI_TILE * PSI_TILE];
    __shared__ T hzi[PSI_TILE * D], hzj[PSI_TILE * D];
    const int tid = threadIdx.x;
    const int share = (int)blockIdx.x / rowblocks, rb = (int)blockIdx.x - share * rowblocks;
    const int i = rb * 256 + tid;
    const bool live = i < n;
    T mv[D], rv[D], il2[D], am[D], aq[D], a0 = (T)0;
    const T c0 = psi2_own_row<T, D, RS>(rc, i, live, ell, mv, rv, il2);
#pragma unroll
    for (int e = 0; e < D; ++e) am[e] = aq[e] = (T)0;
    for (int tile = share; tile < tiles; tile += shares) {
        int ti, tj;
        psi2_tile_of(tile, tiles1d, ti, tj);
        const int i0 = ti * PSI_TILE, j0 = tj * PSI_TILE;
        __syncthreads();                                          // the previous tile has been read
        psi2_stage_points<T, D>(z, m, i0, j0, hzi, hzj, tid);
        __syncthreads();
        // the weights: w g2_jk sf2^2 exp(-delta_jk), delta = sum (z_j / 2 - z_k / 2)^2 / l^2; 0 outside k <= j < m
#pragma unroll 4
        for (int u = 0; u < PSI_TILE * PSI_TILE / 256; ++u) {
            const int el = tid + 256 * u, a = el >> 6, b = el & 63;
            const int gj = i0 + a, gk = j0 + b;
            T v = (T)0;
            if (gj < m && gk <= gj) {
                T zx = (T)0;
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    const T df = hzi[a * D + e] - hzj[b * D + e];
                    zx = fma(df * df, il2[e], zx);
                }
                v = (gj == gk ? (T)1 : (T)2) * g2[(int64_t)gj * ldg + gk] * (sf4 * t_exp(-zx));
            }
            w[el] = v;
        }
        lds_settle(w + tid + 256 * (PSI_TILE * PSI_TILE / 256 - 1));
        __syncthreads();
        if (!live) continue;
        const int na = min(PSI_TILE, m - i0);
        for (int a = 0; a < na; ++a) {
            T di[D];
#pragma unroll
            for (int e = 0; e < D; ++e) di[e] = mv[e] - hzi[a * D + e];
            const int nb = ti == tj ? a + 1 : PSI_TILE;
#pragma unroll 2
            for (int b = 0; b < nb; ++b) {
                T q[D];
                const T ex = psi2_exponent<T, D, true>(c0, di, hzj + b * D, rv, q);
                const T p = w[a * PSI_TILE + b] * t_exp(ex);
                a0 += p;
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    const T pq = p * q[e];
                    am[e] += pq;
                    aq[e] = fma(pq, q[e], aq[e]);
                }
            }
        }
    }
    if (live) {
        T* o = rpart + ((int64_t)share * n + i) * (2 * D);
#pragma unroll
        for (int e = 0; e < D; ++e) {
            o[e] = (T)-2 * am[e];
            o[D + e] = (T)2 * aq[e] - rv[e] * a0;
        }
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_rowreduce(const T* __restrict__ rpart, int n, int shares, T* __restrict__ dmu, T* __restrict__ ds)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * 2 * D) return;
    const int64_t i = idx / (2 * D);
    const int c = (int)(idx - i * (2 * D));
    const T acc = psi_ordered_sum(rpart + idx, shares, (int64_t)n * 2 * D);
    if (c < D) dmu[i * D + c] = acc;
    else       ds[i * D + c - D] = acc;
}

// One tile (ti, tj) of TG x TG pairs and one slice [k0, k1) of the rows.  Thread (ty, tx) owns the points
// i0 + ty + 16 a and j0 + tx + 16 b.  zt: the tile's 2 TG D partial sums of dz (the tile's first-index points, then its
// second-index points); st: its d + 1 partial sums.
template <typename T, int D, bool FULL>
static __device__ __forceinline__ void psi2g_tile(T* __restrict__ lds, T* __restrict__ red, double* __restrict__ sred, const T* __restrict__ z,
                                                  int m, const T* __restrict__ rc, const double* __restrict__ ell, T sf4,
                                                  const T* __restrict__ g2, int64_t ldg, int ti, int tj, int k0, int k1,
                                                  T* __restrict__ zt, double* __restrict__ st)
{
    constexpr int PR = PairGeom<D>::PR, TG = PairGeom<D>::TG, RS = 3 * D + 1;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = ti * TG, j0 = tj * TG;
    const bool diag = ti == tj;
    T hzi[PR][D], hzj[PR][D], wgt[PR][PR], acc[PR][PR], zi[PR][D], zj[PR][D], al[D], il2[D], tl2[D];
#pragma unroll
    for (int e = 0; e < D; ++e) {
        il2[e] = (T)(1.0 / (ell[e] * ell[e]));
        tl2[e] = (T)(2.0 * ell[e] * ell[e]);
        al[e] = (T)0;
    }
    psi2_pair_points<T, D, PR, FULL>(z, m, i0, j0, ty, tx, hzi, hzj);
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int e = 0; e < D; ++e) zi[a][e] = zj[a][e] = (T)0;
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int b = 0; b < PR; ++b) {
            const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * b;
            acc[a][b] = (T)0;
            T v = (T)0;
            if (FULL || (gi < m && gj <= gi)) {
                T zx = (T)0;
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    const T df = hzi[a][e] - hzj[b][e];
                    zx = fma(df * df, il2[e], zx);
                }
                v = (gi == gj ? (T)1 : (T)2) * g2[(int64_t)gi * ldg + gj] * (sf4 * t_exp(-zx));
            }
            wgt[a][b] = v;
        }
    for (int kb = k0; kb < k1; kb += PSI_CHUNK) {
        const int rows = min(PSI_CHUNK, k1 - kb);
        psi2_stage_chunk(lds, rc + (int64_t)kb * RS, rows * RS, tid);
        for (int r = 0; r < rows; ++r) {
            const T* c = lds + r * RS;
            const T c0 = c[3 * D];
#pragma unroll
            for (int a = 0; a < PR; ++a) {
                if (!FULL && i0 + 16 * a >= m) continue;
                T di[D];
#pragma unroll
                for (int e = 0; e < D; ++e) di[e] = c[e] - hzi[a][e];
#pragma unroll
                for (int b = 0; b < PR; ++b) {
                    if (!FULL && (j0 + 16 * b >= m || (diag && b > a))) continue;
                    T q[D];
                    const T ev = t_exp(psi2_exponent<T, D, true>(c0, di, hzj[b], c + D, q));
                    acc[a][b] += ev;
                    const T p = wgt[a][b] * ev;
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        const T pq = p * q[e];
                        zi[a][e] += pq;
                        zj[b][e] += pq;
                        al[e] = fma(p, fma(tl2[e] * q[e], q[e], c[2 * D + e]), al[e]);
                    }
                }
            }
        }
    }
    // the delta parts, which need the pair's own sum: with x = (z_j - z_k) / 2, -+ x / l^2 to dz_j, dz_k and 2 x^2 / l^2 to log l
    T sw = (T)0;
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int b = 0; b < PR; ++b) {
            const T we = wgt[a][b] * acc[a][b];
            sw += we;
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const T x = hzi[a][e] - hzj[b][e], t = we * x * il2[e];
                zi[a][e] -= t;
                zj[b][e] += t;
                al[e] = fma((T)2 * t, x, al[e]);
            }
        }
    // the 16 threads of a thread row (column) hold partial sums of the same first-index (second-index) points: added in
    // thread order.  The barrier that opens the second call is the one that lets red be written again.
    auto add16 = [&](int own, int other, const T (&v)[PR][D], T* __restrict__ out) __attribute__((always_inline)) {
        __syncthreads();
#pragma unroll
        for (int a = 0; a < PR; ++a)
#pragma unroll
            for (int e = 0; e < D; ++e) red[other * (TG * D) + (own + 16 * a) * D + e] = v[a][e];
        lds_settle(red + other * (TG * D) + (own + 16 * (PR - 1)) * D + D - 1);
        __syncthreads();
        for (int idx = tid; idx < TG * D; idx += 256) out[idx] = psi_ordered_sum(red + idx, 16, TG * D);
    };
    add16(ty, tx, zi, zt);
    add16(tx, ty, zj, zt + TG * D);
    const double s0 = block_sum((double)sw, sred);
    if (tid == 0) st[0] = s0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const double se = block_sum((double)al[e], sred);
        if (tid == 0) st[1 + e] = se;
    }
}

// blockIdx.x = tile + tiles * slice
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_pairs(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, const double* __restrict__ ell, T sf4,
                   const T* __restrict__ g2, int64_t ldg, int tiles1d, int tiles, int slice_len, T* __restrict__ zpart,
                   double* __restrict__ spart)
{
    constexpr int TG = PairGeom<D>::TG;
    __shared__ T lds[PSI_CHUNK * (3 * D + 1)];
    __shared__ T red[16 * TG * D];
    __shared__ double sred[16];
    const int slice = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - slice * tiles;
    int ti, tj;
    psi2_tile_of(tile, tiles1d, ti, tj);
    const int k0 = slice * slice_len, k1 = min(n, k0 + slice_len);
    T* zt = zpart + ((int64_t)slice * tiles + tile) * (2 * TG * D);
    double* st = spart + ((int64_t)slice * tiles + tile) * (D + 1);
    if (ti != tj && (ti + 1) * TG <= m) psi2g_tile<T, D, true>(lds, red, sred, z, m, rc, ell, sf4, g2, ldg, ti, tj, k0, k1, zt, st);
    else                                psi2g_tile<T, D, false>(lds, red, sred, z, m, rc, ell, sf4, g2, ldg, ti, tj, k0, k1, zt, st);
}

// blockIdx.x < ceil(m D / 256): one entry of dz per thread; the last workgroup: sums (sums[0] doubled: d / dlog sf2 of
// sf2^2) and the count of bad rows
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_pairreduce(const T* __restrict__ zpart, const double* __restrict__ spart, int m, int tiles1d, int tiles, int slices,
                        T* __restrict__ dz, double* __restrict__ sums, const double* __restrict__ badpart, int nbad, double* __restrict__ bad)
{
    constexpr int TG = PairGeom<D>::TG;
    __shared__ double red[(D + 1) * 256];
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        add_sums<D>(spart, slices * tiles, 2.0, red, tid, sums);
        __syncthreads();
        psi2_count_bad(badpart, nbad, red, tid, bad);
        return;
    }
    const int idx = (int)blockIdx.x * 256 + tid;
    if (idx >= m * D) return;
    const int j = idx / D, e = idx - j * D;
    const int tq = j / TG, off = (j - tq * TG) * D + e;
    T acc = (T)0;
    for (int sl = 0; sl < slices; ++sl) {
        const T* base = zpart + (int64_t)sl * tiles * (2 * TG * D);
        for (int c = 0; c <= tq; ++c) {                          // the tiles (tq, c): j is a first-index point
            const int tile = c * tiles1d - c * (c - 1) / 2 + (tq - c);
            acc += base[(int64_t)tile * (2 * TG * D) + off];
        }
        const int first = tq * tiles1d - tq * (tq - 1) / 2;
        for (int r = tq; r < tiles1d; ++r)                       // the tiles (r, tq): j is a second-index point
            acc += base[(int64_t)(first + r - tq) * (2 * TG * D) + TG * D + off];
    }
    dz[idx] = acc;
}

template <typename T>
static int psi1g_run(int dtype, const T* mu, const T* s, const T* z, int64_t n, int64_t m, int d, const double* ell, double sf2, const T* g1,
                     int64_t ldg, T* dmu, T* ds, T* dz, double* sums, char* scratch, hipStream_t st, const char* fn)
{
    const int64_t cbs = psi1g_colblocks(m), len = psi1g_slice_len(n, m), slices = psi_slice_count(n, len);
    T* zpart = reinterpret_cast<T*>(scratch);
    double* spart = reinterpret_cast<double*>(scratch + psi1g_scratch(dtype, n, m, d).spart);
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi1g_rows<T, D>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, mu, s, z, (int)n, (int)m, ell, (T)sf2, g1,
                           ldg, dmu, ds);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi1g_cols<T, D>), dim3((unsigned)(cbs * slices)), dim3(64), 0, st, mu, s, z, (int)n, (int)m, ell, (T)sf2, g1,
                           ldg, (int)cbs, (int)len, zpart, spart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi1g_reduce<T, D>), dim3((unsigned)((m * D + 255) / 256 + 1)), dim3(256), 0, st, (const T*)zpart,
                           (const double*)spart, (int)m, (int)slices, (int)(cbs * slices), dz, sums);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

template <typename T>
static int psi2g_run(int dtype, const T* mu, const T* s, const T* z, int64_t n, int64_t m, int d, const double* ell, double sf2, const T* g2,
                     int64_t ldg, T* dmu, T* ds, T* dz, double* sums, char* scratch, double* bad, hipStream_t st, const char* fn)
{
    const int64_t nb = psi2_count_blocks(n), shares = psi2g_shares(n, m), rt1 = psi_tiles_1d(m, PSI_TILE), rtiles = psi_tiles(m, PSI_TILE);
    const int64_t edge = psi2g_edge(d), t1 = psi_tiles_1d(m, edge), tiles = psi_tiles(m, edge);
    const int64_t len = psi2g_slice_len(n, m, d), slices = psi_slice_count(n, len);
    const Psi2GradScratch lay = psi2g_scratch(dtype, n, m, d);
    double* badpart = reinterpret_cast<double*>(scratch);
    T* rc = reinterpret_cast<T*>(scratch + lay.rc);
    T* rpart = reinterpret_cast<T*>(scratch + lay.rpart);
    T* zpart = reinterpret_cast<T*>(scratch + lay.zpart);
    double* spart = reinterpret_cast<double*>(scratch + lay.spart);
    const T sf4 = (T)(sf2 * sf2);
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi2_rows<T, D, true>), dim3((unsigned)nb), dim3(256), 0, st, mu, s, (int)n, ell, rc, badpart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2g_rowpass<T, D>), dim3((unsigned)(nb * shares)), dim3(256), 0, st, z, (int)m, (const T*)rc, (int)n, ell,
                           sf4, g2, ldg, (int)nb, (int)shares, (int)rt1, (int)rtiles, rpart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2g_rowreduce<T, D>), dim3((unsigned)((n * 2 * D + 255) / 256)), dim3(256), 0, st, (const T*)rpart, (int)n,
                           (int)shares, dmu, ds);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2g_pairs<T, D>), dim3((unsigned)(tiles * slices)), dim3(256), 0, st, z, (int)m, (const T*)rc, (int)n, ell,
                           sf4, g2, ldg, (int)t1, (int)tiles, (int)len, zpart, spart);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_psi2g_pairreduce<T, D>), dim3((unsigned)((m * D + 255) / 256 + 1)), dim3(256), 0, st, (const T*)zpart,
                           (const double*)spart, (int)m, (int)t1, (int)tiles, (int)slices, dz, sums, (const double*)badpart, (int)nb, bad);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

size_t cimrgp_psi1_grad_scratch_bytes(int dtype, int64_t n, int64_t m, int d)
{
    if (!dtype_known(dtype) || !psi2_sizes_ok(n, m) || d < 1 || d > MAXD) return 0;
    return (size_t)psi1g_scratch(dtype, n, m, d).total;
}

int cimrgp_psi1_grad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d, const double* ell_dev,
                     double sf2, const void* g1_dev, int64_t ldg, void* dmu_dev, void* ds_dev, void* dz_dev, double* sums_dev,
                     void* scratch_dev, size_t scratch_bytes, void* stream)
{
    const char* fn = "cimrgp_psi1_grad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(mu_dev && s_dev && z_dev && ell_dev && g1_dev && dmu_dev && ds_dev && dz_dev && sums_dev && scratch_dev, fn,
                   "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n <= CIMRGP_PSI2_MAX_N, fn, "n must be in [1, 16777216]");
    CIMRGP_REQUIRE(m >= 1 && m <= CIMRGP_PSI2_MAX_M, fn, "m must be in [1, 16384]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(sf2 > 0.0, fn, "sf2 must be positive");
    CIMRGP_REQUIRE(ldg >= m, fn, "leading dimension too small");
    CIMRGP_REQUIRE(aligned16(scratch_dev), fn, "scratch must be 16-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_psi1_grad_scratch_bytes(dtype, n, m, d), fn, "scratch too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return psi1g_run<T>(dtype, (const T*)mu_dev, (const T*)s_dev, (const T*)z_dev, n, m, d, ell_dev, sf2, (const T*)g1_dev, ldg,
                            (T*)dmu_dev, (T*)ds_dev, (T*)dz_dev, sums_dev, (char*)scratch_dev, stream_of(stream), fn);
    });
}

size_t cimrgp_psi2_grad_scratch_bytes(int dtype, int64_t n, int64_t m, int d)
{
    if (!dtype_known(dtype) || !psi2_sizes_ok(n, m) || d < 1 || d > MAXD) return 0;
    return (size_t)psi2g_scratch(dtype, n, m, d).total;
}

int cimrgp_psi2_grad(int dtype, const void* mu_dev, const void* s_dev, const void* z_dev, int64_t n, int64_t m, int d, const double* ell_dev,
                     double sf2, const void* g2_dev, int64_t ldg, void* dmu_dev, void* ds_dev, void* dz_dev, double* sums_dev,
                     void* scratch_dev, size_t scratch_bytes, double* bad_dev, void* stream)
{
    const char* fn = "cimrgp_psi2_grad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(mu_dev && s_dev && z_dev && ell_dev && g2_dev && dmu_dev && ds_dev && dz_dev && sums_dev && scratch_dev && bad_dev, fn,
                   "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n <= CIMRGP_PSI2_MAX_N, fn, "n must be in [1, 16777216]");
    CIMRGP_REQUIRE(m >= 1 && m <= CIMRGP_PSI2_MAX_M, fn, "m must be in [1, 16384]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(sf2 > 0.0, fn, "sf2 must be positive");
    CIMRGP_REQUIRE(ldg >= m, fn, "leading dimension too small");
    CIMRGP_REQUIRE(aligned16(scratch_dev), fn, "scratch must be 16-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_psi2_grad_scratch_bytes(dtype, n, m, d), fn, "scratch too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return psi2g_run<T>(dtype, (const T*)mu_dev, (const T*)s_dev, (const T*)z_dev, n, m, d, ell_dev, sf2, (const T*)g2_dev, ldg,
                            (T*)dmu_dev, (T*)ds_dev, (T*)dz_dev, sums_dev, (char*)scratch_dev, bad_dev, stream_of(stream), fn);
    });
}

}  // extern "C"
