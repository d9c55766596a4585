// The derivatives of the psi statistics contracted with a weight matrix: the calls of include/cimrgp_psi_grad.h.
//   psi1_grad  k_psi1g_rows        a wave per row (wave_row): Psi1 as k_psi1 forms it, lane l takes columns l, l + 64, ..;
//                                  wave_sum of the row's 2 d + 1 sums, lane 0 writes dmu and ds
//              k_psi1g_cols        a thread per column, one wave per workgroup, over one slice of the rows: a chunk's
//                                  row constants are formed by the wave and read back from LDS at one address per
//                                  instruction; partial dz per (slice, column), partial sums per (slice, column block)
//              k_psi1g_reduce      adds the slices in slice order; its last workgroup adds the sums (lds_tree)
//   psi2_grad  k_psi2g_rows        k_psi2_rows with a third constant per dimension, 2 s r (formed in float64: 1 - l^2 r
//                                  would cancel at small s)
//              k_psi2g_rowpass     a thread per row, 256 rows per workgroup, over share p of the 64 x 64 tiles of the
//                                  lower triangle (tiles p, p + P, ..): z / 2 of the tile's points and the weights
//                                  w g2_jk sf2^2 exp(-delta_jk) in LDS, read at one address per instruction
//              k_psi2g_rowreduce   adds the P shares in order: dmu, ds
//              k_psi2g_pairs       k_psi2_tiles' geometry with a tile edge of 16 PR, PR = 4 (d <= 2) or 2: per thread the
//                                  sums of a r for its PR + PR points, of the log-l terms, and of the exponentials per pair
//                                  (the delta parts need Psi2_jk); then the 16 threads of a thread row / column are added
//                                  through LDS in thread order and the d + 1 sums by block_sum
//              k_psi2g_pairreduce  dz_j: slices in slice order, within a slice the tiles that hold point j in tile order;
//                                  its last workgroup adds the sums and the counts of bad rows
// Every hand-over through LDS is: stores, lds_settle on the last word stored, barrier (common.hpp).
// Every partial sum is taken in one fixed order that depends on (n, m, d) alone.
#include "psi_common.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

constexpr int RT = CIMRGP_PSI2_TILE;          // tile edge of the rows pass (pairs)
constexpr int GCHUNK = 64;                    // rows whose constants are staged at a time
template <int D> struct PairGeom {
    static constexpr int PR = D <= 2 ? 4 : 2;                     // pairs per thread and side
    static constexpr int TG = 16 * PR;                            // tile edge: 16 x 16 threads
    static_assert(TG == CIMRGP_PSI_GRAD_PAIR_EDGE(D), "the header's tile edge");
};

// ---- the geometry, functions of (n, m, d) alone ----
static inline int64_t psi1g_colblocks(int64_t m) { return (m + 63) / 64; }
static inline int64_t psi1g_slice_len(int64_t n, int64_t m) { return psi_slice_len(n, psi1g_colblocks(m), CIMRGP_PSI2_TARGET_WGS); }
static inline int64_t psi1g_z_bytes(int dtype, int64_t n, int64_t m, int d)
{
    return round16(psi_slice_count(n, psi1g_slice_len(n, m)) * m * d * (int64_t)elem_bytes(dtype));
}
static inline int64_t psi1g_s_bytes(int64_t n, int64_t m, int d)
{
    return round16(psi_slice_count(n, psi1g_slice_len(n, m)) * psi1g_colblocks(m) * (d + 1) * 8);
}

static inline int64_t psi2g_shares(int64_t n, int64_t m)
{
    int64_t p = CIMRGP_PSI_GRAD_ROW_WGS / psi2_count_blocks(n);
    const int64_t tiles = psi_tiles(m, RT);
    if (p > tiles) p = tiles;
    return p < 1 ? 1 : p;
}
static inline int64_t psi2g_edge(int d) { return CIMRGP_PSI_GRAD_PAIR_EDGE(d); }
static inline int64_t psi2g_slice_len(int64_t n, int64_t m, int d) { return psi_slice_len(n, psi_tiles(m, psi2g_edge(d)), CIMRGP_PSI2_TARGET_WGS); }
static inline int64_t psi2g_rc_bytes(int dtype, int64_t n, int d) { return round16(n * (3 * d + 1) * (int64_t)elem_bytes(dtype)); }
static inline int64_t psi2g_rpart_bytes(int dtype, int64_t n, int64_t m, int d) { return round16(psi2g_shares(n, m) * n * 2 * d * (int64_t)elem_bytes(dtype)); }
static inline int64_t psi2g_units(int64_t n, int64_t m, int d) { return psi_slice_count(n, psi2g_slice_len(n, m, d)) * psi_tiles(m, psi2g_edge(d)); }
static inline int64_t psi2g_zpart_bytes(int dtype, int64_t n, int64_t m, int d)
{
    return round16(psi2g_units(n, m, d) * 2 * psi2g_edge(d) * d * (int64_t)elem_bytes(dtype));
}
static inline int64_t psi2g_spart_bytes(int64_t n, int64_t m, int d) { return round16(psi2g_units(n, m, d) * (d + 1) * 8); }

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
    T mv[D], hr[D];                              // mu_e and 1 / (2 (l_e^2 + s_e)), as k_psi1 has them
    double lg = 0.0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const double sv = (double)s[(int64_t)row * D + e], l2 = ell[e] * ell[e];
        mv[e] = mu[(int64_t)row * D + e];
        hr[e] = (T)(0.5 / (l2 + sv));
        lg += log1p(sv / l2);
    }
    const T c0 = (T)(-0.5 * lg);
    T am[D], aq[D], a0 = (T)0;                   // sum p q_e, sum p q_e^2, sum p: p = g1 Psi1, q_e = (mu_e - z_e) h_e
#pragma unroll
    for (int e = 0; e < D; ++e) am[e] = aq[e] = (T)0;
    const T* grow = g1 + (int64_t)row * ldg;
    for (int j = lane; j < m; j += 64) {
        T ex = c0, df[D];
#pragma unroll
        for (int e = 0; e < D; ++e) {
            df[e] = mv[e] - z[(int64_t)j * D + e];
            ex = fma(-(df[e] * df[e]), hr[e], ex);
        }
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

// blockIdx.x = column block + colblocks * slice; 64 threads.  lds: GCHUNK rows of (mu_e, hr_e, s_e h_e, c0).
template <typename T, int D>
__global__ __launch_bounds__(64)
void k_psi1g_cols(const T* __restrict__ mu, const T* __restrict__ s, const T* __restrict__ z, int n, int m, const double* __restrict__ ell,
                  T sf2, const T* __restrict__ g1, int64_t ldg, int colblocks, int slice_len, T* __restrict__ zpart,
                  double* __restrict__ spart)
{
    constexpr int RS = 3 * D + 1;
    __shared__ T lds[GCHUNK * RS];
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
    for (int kb = k0; kb < k1; kb += GCHUNK) {
        const int rows = min(GCHUNK, k1 - kb);
        __syncthreads();                                          // the previous chunk has been read
        if (tid < rows) {
            const int64_t i = kb + tid;
            T* c = lds + tid * RS;
            double lg = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const double sv = (double)s[i * D + e], ll = ell[e] * ell[e];
                c[e] = mu[i * D + e];
                c[D + e] = (T)(0.5 / (ll + sv));
                c[2 * D + e] = (T)(sv / (ll + sv));
                lg += log1p(sv / ll);
            }
            c[3 * D] = (T)(-0.5 * lg);
            lds_settle(c + 3 * D);
        }
        __syncthreads();
        if (live) {
            for (int r = 0; r < rows; ++r) {
                const T* c = lds + r * RS;
                T ex = c[3 * D], df[D];
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    df[e] = c[e] - zv[e];
                    ex = fma(-(df[e] * df[e]), c[D + e], ex);
                }
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
    T acc = zpart[idx];
    for (int sl = 1; sl < slices; ++sl) acc += zpart[(int64_t)sl * m * D + idx];
    dz[idx] = acc;
}

// ------------------------------------------------------------------ psi2_grad ----
// rc[i] = (mu_i0 .., r_i0 .., 2 s_i0 r_i0 .., c0_i); a bad row gets (0, 0, 0, -inf); badpart[blockIdx.x] = the count.
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_rows(const T* __restrict__ mu, const T* __restrict__ s, int n, const double* __restrict__ ell, T* __restrict__ rc,
                  double* __restrict__ badpart)
{
    constexpr int RS = 3 * D + 1;
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
            o[2 * D + e] = (T)(2.0 * sv / (l2 + 2.0 * sv));
            lg += log1p(2.0 * sv / l2);
        }
        o[3 * D] = (T)(-0.5 * lg);
        if (!ok) {
            bad = 1.0;
#pragma unroll
            for (int k = 0; k < 3 * D; ++k) o[k] = (T)0;
            o[3 * D] = -(T)INFINITY;
        }
#pragma unroll
        for (int k = 0; k < RS; ++k) rc[(int64_t)i * RS + k] = o[k];
    }
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) badpart[blockIdx.x] = bad;
}

// blockIdx.x = row block + rowblocks * share.  rpart[(share n + i) 2 D + ..] = the share's (dmu_i, ds_i).
template <typename T, int D>
__global__ __launch_bounds__(256)
void k_psi2g_rowpass(const T* __restrict__ z, int m, const T* __restrict__ rc, int n, const double* __restrict__ ell, T sf4,
                     const T* __restrict__ g2, int64_t ldg, int rowblocks, int shares, int tiles1d, int tiles, T* __restrict__ rpart)
{
    constexpr int RS = 3 * D + 1;
    __shared__ T w[RT * RT];
    __shared__ T hzi[RT * D], hzj[RT * D];
    const int tid = threadIdx.x;
    const int share = (int)blockIdx.x / rowblocks, rb = (int)blockIdx.x - share * rowblocks;
    const int i = rb * 256 + tid;
    const bool live = i < n;
    T mv[D], rv[D], il2[D], am[D], aq[D], a0 = (T)0;
    const T c0 = live ? rc[(int64_t)i * RS + 3 * D] : -(T)INFINITY;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        mv[e] = live ? rc[(int64_t)i * RS + e] : (T)0;
        rv[e] = live ? rc[(int64_t)i * RS + D + e] : (T)0;
        il2[e] = (T)(1.0 / (ell[e] * ell[e]));
        am[e] = aq[e] = (T)0;
    }
    for (int tile = share; tile < tiles; tile += shares) {
        int ti, tj;
        psi2_tile_of(tile, tiles1d, ti, tj);
        const int i0 = ti * RT, j0 = tj * RT;
        __syncthreads();                                          // the previous tile has been read
        for (int idx = tid; idx < RT * D; idx += 256) {
            const int gi = i0 + idx / D, gj = j0 + idx / D, e = idx % D;
            hzi[idx] = gi < m ? (T)0.5 * z[(int64_t)gi * D + e] : (T)0;
            hzj[idx] = gj < m ? (T)0.5 * z[(int64_t)gj * D + e] : (T)0;
            if (idx + 256 >= RT * D) lds_settle(hzj + idx);
        }
        __syncthreads();
        // the weights: w g2_jk sf2^2 exp(-delta_jk), delta = sum (z_j / 2 - z_k / 2)^2 / l^2; 0 outside k <= j < m
#pragma unroll 4
        for (int u = 0; u < RT * RT / 256; ++u) {
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
        lds_settle(w + tid + 256 * (RT * RT / 256 - 1));
        __syncthreads();
        if (!live) continue;
        const int na = min(RT, m - i0);
        for (int a = 0; a < na; ++a) {
            T di[D];
#pragma unroll
            for (int e = 0; e < D; ++e) di[e] = mv[e] - hzi[a * D + e];
            const int nb = ti == tj ? a + 1 : RT;
#pragma unroll 2
            for (int b = 0; b < nb; ++b) {
                T ex = c0, q[D];
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    const T dl = di[e] - hzj[b * D + e];
                    ex = fma(-(dl * dl), rv[e], ex);
                    q[e] = dl * rv[e];
                }
                const T p = w[a * RT + b] * t_exp(ex);
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
    T acc = rpart[idx];
    for (int p = 1; p < shares; ++p) acc += rpart[(int64_t)p * n * 2 * D + idx];
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
#pragma unroll
    for (int a = 0; a < PR; ++a) {
        const int gi = i0 + ty + 16 * a, gj = j0 + tx + 16 * a;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            hzi[a][e] = (FULL || gi < m) ? (T)0.5 * z[(int64_t)gi * D + e] : (T)0;
            hzj[a][e] = (FULL || gj < m) ? (T)0.5 * z[(int64_t)gj * D + e] : (T)0;
            zi[a][e] = zj[a][e] = (T)0;
        }
    }
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
    for (int kb = k0; kb < k1; kb += GCHUNK) {
        const int rows = min(GCHUNK, k1 - kb);
        __syncthreads();                                          // the previous chunk has been read
        for (int idx = tid; idx < rows * RS; idx += 256) {
            lds[idx] = rc[(int64_t)kb * RS + idx];
            if (idx + 256 >= rows * RS) lds_settle(lds + idx);
        }
        __syncthreads();
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
                    T ex = c0, q[D];
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        const T dl = di[e] - hzj[b][e];
                        ex = fma(-(dl * dl), c[D + e], ex);
                        q[e] = dl * c[D + e];
                    }
                    const T ev = t_exp(ex);
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
    // the 16 threads of a thread row hold partial sums of the same first-index points: added in thread order
    __syncthreads();
#pragma unroll
    for (int a = 0; a < PR; ++a)
#pragma unroll
        for (int e = 0; e < D; ++e) red[tx * (TG * D) + (ty + 16 * a) * D + e] = zi[a][e];
    lds_settle(red + tx * (TG * D) + (ty + 16 * (PR - 1)) * D + D - 1);
    __syncthreads();
    for (int idx = tid; idx < TG * D; idx += 256) {
        T sum = red[idx];
        for (int t = 1; t < 16; ++t) sum += red[t * (TG * D) + idx];
        zt[idx] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < PR; ++b)
#pragma unroll
        for (int e = 0; e < D; ++e) red[ty * (TG * D) + (tx + 16 * b) * D + e] = zj[b][e];
    lds_settle(red + ty * (TG * D) + (tx + 16 * (PR - 1)) * D + D - 1);
    __syncthreads();
    for (int idx = tid; idx < TG * D; idx += 256) {
        T sum = red[idx];
        for (int t = 1; t < 16; ++t) sum += red[t * (TG * D) + idx];
        zt[TG * D + idx] = sum;
    }
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
    __shared__ T lds[GCHUNK * (3 * D + 1)];
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
// sf2^2) and the count of bad rows, as k_psi2_reduce adds it
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
        double b = 0.0;
        for (int i = tid; i < nbad; i += 256) b += badpart[i];
        red[tid] = b;
        lds_tree<256>(red, tid);
        if (tid == 0) bad[0] = red[0];
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
    double* spart = reinterpret_cast<double*>(scratch + psi1g_z_bytes(dtype, n, m, d));
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
    const int64_t nb = psi2_count_blocks(n), shares = psi2g_shares(n, m), rt1 = psi_tiles_1d(m, RT), rtiles = psi_tiles(m, RT);
    const int64_t edge = psi2g_edge(d), t1 = psi_tiles_1d(m, edge), tiles = psi_tiles(m, edge);
    const int64_t len = psi2g_slice_len(n, m, d), slices = psi_slice_count(n, len);
    char* p = scratch;
    double* badpart = reinterpret_cast<double*>(p);  p += psi2_count_bytes(n);
    T* rc = reinterpret_cast<T*>(p);                 p += psi2g_rc_bytes(dtype, n, d);
    T* rpart = reinterpret_cast<T*>(p);              p += psi2g_rpart_bytes(dtype, n, m, d);
    T* zpart = reinterpret_cast<T*>(p);              p += psi2g_zpart_bytes(dtype, n, m, d);
    double* spart = reinterpret_cast<double*>(p);
    const T sf4 = (T)(sf2 * sf2);
    return with_dim_exact(d, [&](auto dd) -> int {
        constexpr int D = decltype(dd)::value;
        hipLaunchKernelGGL((k_psi2g_rows<T, D>), dim3((unsigned)nb), dim3(256), 0, st, mu, s, (int)n, ell, rc, badpart);
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
    return (size_t)(psi1g_z_bytes(dtype, n, m, d) + psi1g_s_bytes(n, m, d));
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
    return (size_t)(psi2_count_bytes(n) + psi2g_rc_bytes(dtype, n, d) + psi2g_rpart_bytes(dtype, n, m, d) + psi2g_zpart_bytes(dtype, n, m, d)
                    + psi2g_spart_bytes(n, m, d));
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
