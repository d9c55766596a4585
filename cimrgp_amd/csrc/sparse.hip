// Inducing-point (sparse) GP regression: the three calls of include/cimrgp_sparse.h and their two twins of
// include/cimrgp_sparse_layer.h, which read the noise, a bias and an extra variance from the device (same kernel bodies),
// and cimrgp_sparse_lambda_kd of include/cimrgp_sparse_linear.h, which reads k(x_i, x_i) per row (same body again).
//   wsyrk_tn       lower(C) = diag_add I + A^T diag(w) A and g = A^T diag(w) r for A (n x m, row-major), n >> m:
//                    k_wsyrk_tn       one 128 x 128 output tile and one slice of K = n per workgroup, on the matrix cores
//                                     (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Mx<T> in common.hpp); the partial
//                                     tile goes to scratch
//                    k_wsyrk_reduce   adds the slices' partials in slice order, adds diag_add, writes lower(C) and g
//                  cimrgp_svgp_moments (include/cimrgp_svgp.h) is the same pair with g = A^T r, r not weighted (RAW)
//   sparse_lambda  k_sparse_rowsq (a wave per row: q_i, lambda_i) and k_sparse_sums (one workgroup: the three sums in a
//                  fixed order, w = 1 / lambda)
//   sparse_tail    k_sparse_tail (a wave per test row: W* gamma, sum A*^2, sum W*^2)
//
// k_wsyrk_tn.  The update kernels of gemm_nt.hip are C -= A B^T with both operands K-contiguous.  Here the K index runs
// down the ROWS of A: a chunk of KC rows of the tile's two column strips (128 columns each, contiguous in memory: the
// global loads coalesce along i) is staged in LDS as it lies in memory, [k][i], and the MFMA fragments are read across
// it: lane l of a 16 x 16 x 4 multiply needs (i = l & 15, k = l >> 4), i.e. 16 consecutive i of 4 consecutive rows; the
// LDS row pitch is 128 elements plus a pad that puts rows k and k + 1 (FP64) / k and k + 2 (FP32, whose k-slot holds
// two k) into different halves of the banks, so a fragment read is conflict-free.  w[k] multiplies the RIGHT operand's
// chunk once, as it is staged.  g rides in the workgroups of tile column 0 (every row tile occurs there once): the
// staged rows of w r form a third, 16-column operand (q <= 8 columns used) and cost the waves of the left half one
// more multiply per row tile and k step.
// Every hand-off through LDS is: stores, lds_settle (read back the last word stored), lds_barrier.
#include "abi.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

constexpr int WS_GT = 128;                    // output tile edge
constexpr int WS_GQ = 16;                     // columns of the g operand (one MFMA tile)
constexpr int WS_SLICE_ALIGN = 32;            // slices start on multiples of the larger chunk (FP32's)
constexpr int WS_TARGET_WGS = 1024;           // tiles x S aims at two rounds of two workgroups per compute unit (256 units)

template <typename T> struct WsGeom {
    static constexpr int KC = 128 / (int)sizeof(T);                    // rows of A per stage: 16 (FP64) / 32 (FP32)
    static constexpr int PAD = sizeof(T) == 8 ? 16 : 8;                // see the bank note above
    static constexpr int PITCH = WS_GT + PAD;                          // elements
    static constexpr int EPC = Mx<T>::EPC;                             // elements per 16-byte chunk
    static constexpr int CPR = WS_GT / EPC;                            // chunks per staged row
    static constexpr int RPP = 256 / CPR;                              // rows per staging pass
    static constexpr int NP = KC / RPP;                                // staging passes (4 for both types)
    static constexpr int OP = KC * PITCH;                              // one operand, one stage (elements)
    static constexpr int GOP = KC * WS_GQ;                             // the g operand, one stage
    static constexpr int GPT = GOP / 256;                              // its elements per thread
};

// S(n, m) and the slice length: a function of n and m alone (not of the dtype, the device or its load).
static inline int64_t ws_tiles_1d(int64_t m) { return (m + WS_GT - 1) / WS_GT; }
static inline int64_t ws_tiles(int64_t m) { const int64_t t = ws_tiles_1d(m); return t * (t + 1) / 2; }
static inline int64_t ws_slice_len(int64_t n, int64_t m)
{
    int64_t s = WS_TARGET_WGS / ws_tiles(m);
    const int64_t smax = (n + 255) / 256;                              // a slice is at least 256 rows
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int64_t len = (n + s - 1) / s;
    return (len + WS_SLICE_ALIGN - 1) / WS_SLICE_ALIGN * WS_SLICE_ALIGN;
}
static inline int64_t ws_slices(int64_t n, int64_t m) { const int64_t len = ws_slice_len(n, m); return (n + len - 1) / len; }

template <typename T> static __device__ __forceinline__ uint4 scale_chunk(uint4 v, T w);
template <> __device__ __forceinline__ uint4 scale_chunk<double>(uint4 v, double w)
{
    const double a = __hiloint2double((int)v.y, (int)v.x) * w, b = __hiloint2double((int)v.w, (int)v.z) * w;
    return make_uint4((unsigned)__double2loint(a), (unsigned)__double2hiint(a), (unsigned)__double2loint(b), (unsigned)__double2hiint(b));
}
template <> __device__ __forceinline__ uint4 scale_chunk<float>(uint4 v, float w)
{
    return make_uint4(__float_as_uint(__uint_as_float(v.x) * w), __float_as_uint(__uint_as_float(v.y) * w),
                      __float_as_uint(__uint_as_float(v.z) * w), __float_as_uint(__uint_as_float(v.w) * w));
}

// One 16-byte chunk of row `row` of A at column `col` (a multiple of EPC) for an EDGE tile: the columns < mcols of it,
// zeros beyond; no element at a column >= mcols is read.
template <typename T>
static __device__ __forceinline__ uint4 load_chunk_edge(const T* __restrict__ row, int col, int mcols)
{
    constexpr int EPC = Mx<T>::EPC;
    if (col + EPC <= mcols) return *reinterpret_cast<const uint4*>(row + col);
    T v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = (col + e < mcols) ? row[col + e] : (T)0;
    uint4 out;
    __builtin_memcpy(&out, v, 16);
    return out;
}

// The k-slot of one fragment: the EPS elements at rows k, k + 1 (FP32) of column i of a staged operand.
template <typename T>
static __device__ __forceinline__ uint2 frag(const T* __restrict__ op, int pitch, int k, int i)
{
    if constexpr (sizeof(T) == 8) {
        const double v = op[k * pitch + i];
        return make_uint2((unsigned)__double2loint(v), (unsigned)__double2hiint(v));
    } else {
        return make_uint2(__float_as_uint(op[k * pitch + i]), __float_as_uint(op[(k + 1) * pitch + i]));
    }
}

// blockIdx.x = tile + tiles * slice; tiles run down the columns of the lower triangle: (0,0) (1,0) .. (t-1,0) (1,1) ..
// EDGE: the tile touches column m or the slice touches row n (ragged m, the last slice): bounds logic on every load.
// RAW (cimrgp_svgp_moments, include/cimrgp_svgp.h): the g operand is r itself, not w r.
template <typename T, bool EDGE, bool RAW>
static __device__ __forceinline__ void wsyrk_tile(T* __restrict__ smem, const T* __restrict__ A, int64_t lda, int n, int m,
                                                  const T* __restrict__ w, const T* __restrict__ r, int q, int ti, int tj, int k0,
                                                  int k1, T* __restrict__ ctile, T* __restrict__ gtile)
{
    using X = Mx<T>;
    using G = WsGeom<T>;
    using acc_t = typename X::acc_t;
    constexpr int KC = G::KC, NP = G::NP, PITCH = G::PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const bool diag = ti == tj;
    const bool do_g = gtile != nullptr;
    const int i0 = ti * WS_GT, j0 = tj * WS_GT;

    const int sc = tid % G::CPR, sr = tid / G::CPR;
    const int ccol = sc * G::EPC;                       // this thread's chunk: column inside the tile
    const int nkt = (k1 - k0 + KC - 1) / KC;

    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    uint4 ra[NP], rb[NP];
    T rw[NP];
    T rg[G::GPT];
#pragma unroll
    for (int p = 0; p < NP; ++p) rb[p] = zero4;          // a diagonal tile never loads it

    auto gload = [&](int kt) {
        const int kb = k0 + kt * KC;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int k = kb + sr + p * G::RPP;
            if (EDGE) {
                if (k < k1) {
                    const T* row = A + (int64_t)k * lda;
                    ra[p] = (i0 + ccol < m) ? load_chunk_edge<T>(row, i0 + ccol, m) : zero4;
                    if (!diag) rb[p] = (j0 + ccol < m) ? load_chunk_edge<T>(row, j0 + ccol, m) : zero4;
                    rw[p] = w[k];
                } else {
                    ra[p] = zero4;
                    rb[p] = zero4;
                    rw[p] = (T)0;
                }
            } else {
                const T* row = A + (int64_t)k * lda;
                ra[p] = *reinterpret_cast<const uint4*>(row + i0 + ccol);
                if (!diag) rb[p] = *reinterpret_cast<const uint4*>(row + j0 + ccol);
                rw[p] = w[k];
            }
        }
        if (do_g) {
#pragma unroll
            for (int e = 0; e < G::GPT; ++e) {
                const int idx = tid + 256 * e, kk = kb + idx / WS_GQ, c = idx % WS_GQ;
                if constexpr (RAW) rg[e] = (c < q && kk < k1) ? r[(int64_t)kk * q + c] : (T)0;
                else rg[e] = (c < q && kk < k1) ? w[kk] * r[(int64_t)kk * q + c] : (T)0;
            }
        }
    };
    auto swrite = [&](int buf) {
        T* as = smem + buf * (2 * G::OP + G::GOP);
        T* bs = as + G::OP;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int off = (sr + p * G::RPP) * PITCH + ccol;
            *reinterpret_cast<uint4*>(as + off) = ra[p];
            *reinterpret_cast<uint4*>(bs + off) = scale_chunk<T>(diag ? ra[p] : rb[p], rw[p]);
        }
        if (do_g) {
            T* gs = bs + G::OP;
#pragma unroll
            for (int e = 0; e < G::GPT; ++e) gs[tid + 256 * e] = rg[e];
        }
        lds_settle(bs + (sr + (NP - 1) * G::RPP) * PITCH + ccol);
    };

    acc_t acc[4][4], accg[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        accg[mi] = acc_zero<T>();
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = acc_zero<T>();
    }
    const int frow = lane & 15, fslot = lane >> 4;
    constexpr int KSTEP = 4 * X::EPS;

    gload(0);
    swrite(0);
    lds_barrier();
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = kt + 1 < nkt;
        if (more) gload(kt + 1);
        const T* as = smem + (kt & 1) * (2 * G::OP + G::GOP);
        const T* bs = as + G::OP;
        const T* gs = bs + G::OP;
#pragma unroll
        for (int s = 0; s < KC / KSTEP; ++s) {
            const int k = s * KSTEP + fslot * X::EPS;
            uint2 a[4], b[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) a[mi] = frag<T>(as, PITCH, k, wr * 64 + mi * 16 + frow);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) b[ni] = frag<T>(bs, PITCH, k, wc * 64 + ni * 16 + frow);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = X::mma(a[mi], b[ni], acc[mi][ni]);
            if (do_g && wc == 0) {
                const uint2 bg = frag<T>(gs, WS_GQ, k, frow);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) accg[mi] = X::mma(a[mi], bg, accg[mi]);
            }
        }
        if (more) swrite((kt + 1) & 1);
        lds_barrier();
    }

    // the partial tile, 128 x 128 row-major (whole tiles: no bounds), and the partial g rows (128 x 8)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int c = wc * 64 + ni * 16 + (lane & 15);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) ctile[(wr * 64 + mi * 16 + X::crow(lane, rr)) * WS_GT + c] = acc[mi][ni][rr];
        }
    }
    if (do_g && wc == 0 && (lane & 15) < MAXQ) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) gtile[(wr * 64 + mi * 16 + X::crow(lane, rr)) * MAXQ + (lane & 15)] = accg[mi][rr];
    }
}

template <typename T, bool RAW = false>
__global__ __launch_bounds__(256, 2)
void k_wsyrk_tn(const T* __restrict__ A, int64_t lda, int n, int m, const T* __restrict__ w, const T* __restrict__ r, int q,
                int tiles1d, int tiles, int slice_len, T* __restrict__ cpart, T* __restrict__ gpart)
{
    using G = WsGeom<T>;
    __shared__ __attribute__((aligned(16))) T smem[2 * (2 * G::OP + G::GOP)];
    const int slice = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - slice * tiles;
    // column tj of the triangle holds tiles1d - tj tiles, the diagonal one first
    int tj = 0, first = 0;
    while (tile >= first + (tiles1d - tj)) { first += tiles1d - tj; ++tj; }
    const int ti = tj + (tile - first);
    const int k0 = slice * slice_len, k1 = min(n, k0 + slice_len);
    T* ctile = cpart + ((int64_t)slice * tiles + tile) * (WS_GT * WS_GT);
    T* gtile = (r != nullptr && tj == 0) ? gpart + ((int64_t)slice * tiles1d + ti) * (WS_GT * MAXQ) : nullptr;
    const bool edge = (ti + 1) * WS_GT > m || (k1 - k0) % G::KC != 0;
    if (edge) wsyrk_tile<T, true, RAW>(smem, A, lda, n, m, w, r, q, ti, tj, k0, k1, ctile, gtile);
    else      wsyrk_tile<T, false, RAW>(smem, A, lda, n, m, w, r, q, ti, tj, k0, k1, ctile, gtile);
}

// blockIdx.x < tiles * 64: 256 elements of one tile (two rows of it); beyond: 256 elements of g.  Slices are added in
// the order 0, 1, ..: a fixed order.  Only j <= i of C is written.
template <typename T>
__global__ __launch_bounds__(256)
void k_wsyrk_reduce(const T* __restrict__ cpart, const T* __restrict__ gpart, int m, int q, int tiles1d, int tiles, int slices,
                    T diag_add, T* __restrict__ C, int64_t ldc, T* __restrict__ g)
{
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < tiles * 64) {
        const int tile = (int)blockIdx.x >> 6, part = (int)blockIdx.x & 63;
        int tj = 0, first = 0;
        while (tile >= first + (tiles1d - tj)) { first += tiles1d - tj; ++tj; }
        const int ti = tj + (tile - first);
        const int e = part * 256 + tid;
        const int i = ti * WS_GT + (e >> 7), j = tj * WS_GT + (e & 127);
        if (i >= m || j > i) return;
        const T* p = cpart + (int64_t)tile * (WS_GT * WS_GT) + e;
        T s = p[0];
        for (int sl = 1; sl < slices; ++sl) s += p[(int64_t)sl * tiles * (WS_GT * WS_GT)];
        C[(int64_t)i * ldc + j] = (i == j) ? s + diag_add : s;
    } else {
        const int e = ((int)blockIdx.x - tiles * 64) * 256 + tid;
        if (e >= m * q) return;
        const int i = e / q, c = e - i * q;
        const T* p = gpart + (int64_t)i * MAXQ + c;
        T s = p[0];
        for (int sl = 1; sl < slices; ++sl) s += p[(int64_t)sl * tiles1d * (WS_GT * MAXQ)];
        g[e] = s;
    }
}

// --------------------------------------------------------------------- lambda ----
// A wave per row (wave_row, reduce.hpp): lane l adds the squares of columns l, l + 64, .. in FP64, then the 64 partial
// sums are added pairwise (wave_sum: xor 32, 16, .. 1): a fixed order.  lam <- lambda_i, dtmp <- sf2 - q_i
// (k_sparse_sums turns it into w).  noise_dev != nullptr: the noise is that element on the device, not the argument.
// kdiag != nullptr (cimrgp_sparse_lambda_kd): k(x_i, x_i) is kdiag[i], not the constant sf2.
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_rowsq(const T* __restrict__ A, int64_t lda, int n, int m, double sf2, double noise, const T* __restrict__ noise_dev,
                    const T* __restrict__ kdiag, int mode, T* __restrict__ lam, T* __restrict__ dtmp)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    const T* a = A + (int64_t)row * lda;
    double s = 0.0;
    for (int c = lane; c < m; c += 64) {
        const double v = (double)a[c];
        s += v * v;
    }
    wave_sum(s);
    if (lane == 0) {
        if (noise_dev) noise = (double)noise_dev[0];
        const double d = (kdiag ? (double)kdiag[row] : sf2) - s;
        lam[row] = (T)(mode == 0 ? d + noise : noise);
        dtmp[row] = (T)d;
    }
}

// One workgroup of 1024 threads: thread t takes i = t, t + 1024, ..; the 1024 partial sums are added pairwise in LDS
// (lds_tree, reduce.hpp).
template <typename T>
__global__ __launch_bounds__(1024)
void k_sparse_sums(const T* __restrict__ lam, T* __restrict__ w, int n, double* __restrict__ sums)
{
    __shared__ double red[3][1024];
    const int tid = threadIdx.x;
    double slog = 0.0, sd = 0.0, bad = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const T l = lam[i];
        sd += (double)w[i];
        slog += log((double)l);
        if (!(l > (T)0)) bad += 1.0;
        w[i] = (T)1 / l;
    }
    red[0][tid] = slog;
    red[1][tid] = sd;
    red[2][tid] = bad;
    lds_tree<1024, 3>(&red[0][0], tid);
    if (tid < 3) sums[tid] = red[tid][0];
}

// ----------------------------------------------------------------------- tail ----
// The row walk of k_sparse_rowsq (wave_row, wave_sum).  bias (q elements) and extra (one element) may be nullptr: then
// they add nothing and the result is that of the call without them, bit for bit.  Both are added in FP64 before the one
// rounding to T.
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_tail(const T* __restrict__ As, const T* __restrict__ Ws, int ns, int m, int64_t lda, const T* __restrict__ gamma, int q,
                   double base, const T* __restrict__ bias, const T* __restrict__ extra, T* __restrict__ mean, T* __restrict__ var,
                   int accumulate)
{
    int row, lane;
    if (!wave_row(ns, row, lane)) return;
    double sa = 0.0, sw = 0.0, acc[MAXQ] = {};
    const T* wrow = Ws + (int64_t)row * lda;
    for (int j = lane; j < m; j += 64) {
        const double wv = (double)wrow[j];
        if (var) {
            const double av = (double)As[(int64_t)row * lda + j];
            sa += av * av;
            sw += wv * wv;
        }
        if (mean) dot_step(acc, wv, gamma + (int64_t)j * q, q);
    }
    wave_sum(sa, sw, acc);
    if (lane != 0) return;
    if (var) {
        if (extra) base += (double)extra[0];
        put(var + row, (T)(base - sa + sw), accumulate);
    }
    if (mean) {
#pragma unroll
        for (int c = 0; c < MAXQ; ++c)
            if (c < q) put(mean + (int64_t)row * q + c, bias ? (T)(acc[c] + (double)bias[c]) : (T)acc[c], accumulate);
    }
}

static inline bool ws_sizes_ok(int64_t n, int64_t m) { return n >= 1 && n <= CIMRGP_WSYRK_MAX_N && m >= 1 && m <= CIMRGP_WSYRK_MAX_M; }

// elements of scratch: the partial tiles, then the partial g
static inline int64_t ws_cpart_elems(int64_t n, int64_t m) { return ws_slices(n, m) * ws_tiles(m) * (WS_GT * WS_GT); }
static inline int64_t ws_gpart_elems(int64_t n, int64_t m) { return ws_slices(n, m) * ws_tiles_1d(m) * (WS_GT * MAXQ); }

}  // namespace

template <typename T, bool RAW = false>
static int wsyrk_tn_run(const T* a, int64_t n, int64_t m, int64_t lda, const T* w, const T* r, int q, double diag_add, T* c, int64_t ldc,
                        T* g, T* scratch, hipStream_t st, const char* fn)
{
    const int64_t t1 = ws_tiles_1d(m), tiles = ws_tiles(m), len = ws_slice_len(n, m), slices = ws_slices(n, m);
    T* cpart = scratch;
    T* gpart = scratch + ws_cpart_elems(n, m);
    hipLaunchKernelGGL((k_wsyrk_tn<T, RAW>), dim3((unsigned)(tiles * slices)), dim3(256), 0, st, a, lda, (int)n, (int)m, w, r, q, (int)t1,
                       (int)tiles, (int)len, cpart, gpart);
    CIMRGP_LAUNCH_CHECK(fn);
    const int64_t gblocks = r ? (m * q + 255) / 256 : 0;
    hipLaunchKernelGGL((k_wsyrk_reduce<T>), dim3((unsigned)(tiles * 64 + gblocks)), dim3(256), 0, st, (const T*)cpart, (const T*)gpart,
                       (int)m, q, (int)t1, (int)tiles, (int)slices, (T)diag_add, c, ldc, g);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

size_t cimrgp_wsyrk_tn_scratch_bytes(int dtype, int64_t n, int64_t m, int q)
{
    if (!dtype_known(dtype) || !ws_sizes_ok(n, m) || q < 0 || q > MAXQ) return 0;
    return (size_t)(ws_cpart_elems(n, m) + (q > 0 ? ws_gpart_elems(n, m) : 0)) * elem_bytes(dtype);
}

// cimrgp_wsyrk_tn and, with `raw` (g = A^T r, r not weighted), cimrgp_svgp_moments (include/cimrgp_svgp.h).  Without r the
// two are the same launch of the same instance.
static int wsyrk_tn_impl(const char* fn, bool raw, int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* w_dev,
                         const void* r_dev, int q, double diag_add, void* c_dev, int64_t ldc, void* g_dev, void* scratch_dev,
                         size_t scratch_bytes, void* stream)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(a_dev && w_dev && c_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(r_dev == nullptr || g_dev != nullptr, fn, "null pointer (g)");
    CIMRGP_REQUIRE(n >= 1 && n <= CIMRGP_WSYRK_MAX_N, fn, "n must be in [1, 16777216]");
    CIMRGP_REQUIRE(m >= 1 && m <= CIMRGP_WSYRK_MAX_M, fn, "m must be in [1, 16384]");
    CIMRGP_REQUIRE(r_dev == nullptr || (q >= 1 && q <= MAXQ), fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(lda >= m && ldc >= m, fn, "leading dimension too small");
    CIMRGP_REQUIRE(lda % elems_per_16_bytes(dtype) == 0, fn, "lda must be a multiple of 16 bytes");
    CIMRGP_REQUIRE(aligned16(a_dev) && aligned16(scratch_dev), fn, "pointers must be 16-byte aligned");
    if (r_dev == nullptr) q = 0;
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_wsyrk_tn_scratch_bytes(dtype, n, m, q), fn, "scratch too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        if (raw && r_dev != nullptr)
            return wsyrk_tn_run<T, true>((const T*)a_dev, n, m, lda, (const T*)w_dev, (const T*)r_dev, q, diag_add, (T*)c_dev, ldc,
                                         (T*)g_dev, (T*)scratch_dev, stream_of(stream), fn);
        return wsyrk_tn_run<T>((const T*)a_dev, n, m, lda, (const T*)w_dev, (const T*)r_dev, q, diag_add, (T*)c_dev, ldc, (T*)g_dev,
                               (T*)scratch_dev, stream_of(stream), fn);
    });
}

int cimrgp_wsyrk_tn(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* w_dev, const void* r_dev, int q,
                    double diag_add, void* c_dev, int64_t ldc, void* g_dev, void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return wsyrk_tn_impl("cimrgp_wsyrk_tn", false, dtype, a_dev, n, m, lda, w_dev, r_dev, q, diag_add, c_dev, ldc, g_dev, scratch_dev,
                         scratch_bytes, stream);
}

size_t cimrgp_svgp_moments_scratch_bytes(int dtype, int64_t n, int64_t m, int q)
{
    return cimrgp_wsyrk_tn_scratch_bytes(dtype, n, m, q);
}

int cimrgp_svgp_moments(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* w_dev, const void* r_dev, int q,
                        void* c_dev, int64_t ldc, void* g_dev, void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return wsyrk_tn_impl("cimrgp_svgp_moments", true, dtype, a_dev, n, m, lda, w_dev, r_dev, q, 0.0, c_dev, ldc, g_dev, scratch_dev,
                         scratch_bytes, stream);
}

// cimrgp_sparse_lambda and cimrgp_sparse_lambda_dev: `dev_entry` says which; the first takes `noise`, the second noise_dev.
// cimrgp_sparse_lambda_kd (include/cimrgp_sparse_linear.h): `kd_entry`, with kdiag_dev in place of sf2.
static int sparse_lambda_impl(const char* fn, bool dev_entry, int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, double sf2,
                              double noise, const void* noise_dev, int mode, void* lam_dev, void* w_dev, double* sums_dev, void* stream,
                              bool kd_entry = false, const void* kdiag_dev = nullptr)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(a_dev && lam_dev && w_dev && sums_dev, fn, "null pointer");
    CIMRGP_REQUIRE(!dev_entry || noise_dev, fn, "null pointer (noise)");
    CIMRGP_REQUIRE(!kd_entry || kdiag_dev, fn, "null pointer (kdiag)");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 31) && m >= 1 && m < (1ll << 31) && lda >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(mode == 0 || mode == 1, fn, "mode must be 0 (FITC) or 1 (VFE)");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_rowsq<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)a_dev, lda, (int)n,
                           (int)m, sf2, noise, (const T*)noise_dev, (const T*)kdiag_dev, mode, (T*)lam_dev, (T*)w_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_sparse_sums<T>), dim3(1), dim3(1024), 0, stream_of(stream), (const T*)lam_dev, (T*)w_dev, (int)n, sums_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

// cimrgp_sparse_tail (bias_dev and extra_var_dev nullptr) and cimrgp_sparse_tail_dev.
static int sparse_tail_impl(const char* fn, int dtype, const void* astar_dev, const void* wstar_dev, int64_t ns, int64_t m, int64_t lda,
                            const void* gamma_dev, int q, double sf2, double extra_var, const void* bias_dev, const void* extra_var_dev,
                            void* mean_dev, void* var_dev, int accumulate, void* stream)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(wstar_dev, fn, "null pointer");
    CIMRGP_REQUIRE(var_dev == nullptr || astar_dev, fn, "null pointer (astar)");
    CIMRGP_REQUIRE(mean_dev == nullptr || gamma_dev, fn, "null pointer (gamma)");
    CIMRGP_REQUIRE(ns >= 0 && ns < (1ll << 31) && m >= 1 && m < (1ll << 31) && lda >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(mean_dev == nullptr || (q >= 1 && q <= MAXQ), fn, "number of outputs must be in [1, 8]");
    if (ns == 0 || (mean_dev == nullptr && var_dev == nullptr)) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_tail<T>), dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)astar_dev,
                           (const T*)wstar_dev, (int)ns, (int)m, lda, (const T*)gamma_dev, q, sf2 + extra_var, (const T*)bias_dev,
                           (const T*)extra_var_dev, (T*)mean_dev, (T*)var_dev, accumulate);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

int cimrgp_sparse_lambda(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, double sf2, double noise, int mode,
                         void* lam_dev, void* w_dev, double* sums_dev, void* stream)
{
    return sparse_lambda_impl("cimrgp_sparse_lambda", false, dtype, a_dev, n, m, lda, sf2, noise, nullptr, mode, lam_dev, w_dev, sums_dev,
                              stream);
}

int cimrgp_sparse_lambda_dev(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, double sf2, const void* noise_dev, int mode,
                             void* lam_dev, void* w_dev, double* sums_dev, void* stream)
{
    return sparse_lambda_impl("cimrgp_sparse_lambda_dev", true, dtype, a_dev, n, m, lda, sf2, 0.0, noise_dev, mode, lam_dev, w_dev,
                              sums_dev, stream);
}

int cimrgp_sparse_lambda_kd(int dtype, const void* a_dev, int64_t n, int64_t m, int64_t lda, const void* kdiag_dev, double noise, int mode,
                            void* lam_dev, void* w_dev, double* sums_dev, void* stream)
{
    return sparse_lambda_impl("cimrgp_sparse_lambda_kd", false, dtype, a_dev, n, m, lda, 0.0, noise, nullptr, mode, lam_dev, w_dev, sums_dev,
                              stream, true, kdiag_dev);
}

int cimrgp_sparse_tail(int dtype, const void* astar_dev, const void* wstar_dev, int64_t ns, int64_t m, int64_t lda,
                       const void* gamma_dev, int q, double sf2, double extra_var, void* mean_dev, void* var_dev, int accumulate,
                       void* stream)
{
    return sparse_tail_impl("cimrgp_sparse_tail", dtype, astar_dev, wstar_dev, ns, m, lda, gamma_dev, q, sf2, extra_var, nullptr, nullptr,
                            mean_dev, var_dev, accumulate, stream);
}

int cimrgp_sparse_tail_dev(int dtype, const void* astar_dev, const void* wstar_dev, int64_t ns, int64_t m, int64_t lda,
                           const void* gamma_dev, int q, double sf2, double extra_var, const void* bias_dev, const void* extra_var_dev,
                           void* mean_dev, void* var_dev, int accumulate, void* stream)
{
    return sparse_tail_impl("cimrgp_sparse_tail_dev", dtype, astar_dev, wstar_dev, ns, m, lda, gamma_dev, q, sf2, extra_var, bias_dev,
                            extra_var_dev, mean_dev, var_dev, accumulate, stream);
}

}  // extern "C"
