// Gradients of the sparse (inducing-point) objective: the three calls of include/cimrgp_sparse_grad.h, the ARD twin of the
// first (include/cimrgp_sparse_ard.h) and its twin with a linear term (include/cimrgp_sparse_linear.h).
//   cov_pair_grad        k_cov_pair_grad    one tile of 128 columns of G and one slice of its rows per workgroup: k, g and
//                                           dk/dlog l recomputed per pair, the products with G and every sum in FP64;
//                                           the partial db and the two partial scalar sums go to scratch
//                        k_pair_grad_reduce adds the partials in slice (and tile) order, applies scale / accumulate
//   cov_pair_grad_ard    the ARD arm of k_cov_pair_grad: 1 + d scalar sums (sum G k, then sum G g (xa_e - xb_e)^2 per
//                                           dimension e) in place of the two; the same reduce kernel
//   sparse_grad_rows     k_sparse_grad_rows (a wave per row: V_i gamma, |V_i|^2 -> beta_i, h_i) and k_sparse_grad_sums
//                                           (one workgroup: the two sums in a fixed order, t)
//   sparse_grad_combine  k_sparse_grad_combine (a wave per row, in place on Y)
//
// k_cov_pair_grad.  The layout is the cross-Gram kernel's (gram.hip) read instead of written: a lane owns the 16 bytes
// of a row of G it loads with ONE instruction -- EPL = 2 doubles / 4 floats -- and the lanes of a wave are adjacent
// along the row, so every load instruction reads whole 512-byte runs (1 row x 64 lanes in FP64, 2 rows x 32 lanes in
// FP32).  The lane's EPL points of xb stay in registers for the whole slice, its EPL x d sums of db too; the row's
// point of xa is the same address for every lane of the row (one request).  The next row's G chunk and xa point are
// loaded before the current row's exponentials.  A chunk that straddles column nb, or is not 16-byte aligned, is read
// element by element: no column >= nb and no row >= na of G is read.
// The ARD arm keeps d more FP64 sums per lane, sum G g df_e^2 (= sum G dk/dlog l_e at equal length-scales), in place of
// sum G dk/dlog l: the product wg df_e that db adds is multiplied by df_e once more.  k, g and db are the same
// instructions in both arms.
// The LIN arm (cimrgp_cov_pair_grad_lin, include/cimrgp_sparse_linear.h: k = k_cov + sum_e lin_e a_e b_e) keeps EPL x d more
// FP64 sums per lane, P_je = sum_i G_ij xa_ie, filled from the same single read of G; their partials go to scratch beside
// the partial db, and the LIN arm of the reduce kernel folds them into db (lin_e P_je) and into lsums (sum_j xb_je P_je).
// k, g, the scalar sums and the covariance part of db are the same instructions as without it.
#include "abi.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

constexpr int PG_CT = 128;                    // columns of G per workgroup
constexpr int PG_TARGET_WGS = 1024;           // tiles x S aims at four workgroups per compute unit (256 units)
constexpr int PG_SLICE_ALIGN = 8;             // rows of G per pass of a workgroup (4 waves x 2 rows in FP32)

// S(na, nb) and the slice length: a function of na and nb alone (not of the dtype, the device or its load).
static inline int64_t pg_tiles(int64_t nb) { return (nb + PG_CT - 1) / PG_CT; }
static inline int64_t pg_slice_len(int64_t na, int64_t nb)
{
    int64_t s = PG_TARGET_WGS / pg_tiles(nb);
    const int64_t smax = (na + 255) / 256;                             // a slice is at least 256 rows
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    const int64_t len = (na + s - 1) / s;
    return (len + PG_SLICE_ALIGN - 1) / PG_SLICE_ALIGN * PG_SLICE_ALIGN;
}
static inline int64_t pg_slices(int64_t na, int64_t nb) { const int64_t len = pg_slice_len(na, nb); return (na + len - 1) / len; }
static inline bool pg_sizes_ok(int64_t na, int64_t nb, int d)
{
    return na >= 1 && na <= CIMRGP_PAIR_GRAD_MAX_NA && nb >= 1 && nb <= CIMRGP_PAIR_GRAD_MAX_NB && d >= 1 && d <= MAXD;
}
// doubles of scratch: the partial db, then the partial sums
static inline int64_t pg_dbpart_elems(int64_t na, int64_t nb, int d) { return pg_slices(na, nb) * pg_tiles(nb) * PG_CT * d; }
static inline int64_t pg_sumpart_elems(int64_t na, int64_t nb, int nsums) { return pg_slices(na, nb) * pg_tiles(nb) * nsums; }
static inline int pg_nsums(int d, bool ard) { return ard ? 1 + d : 2; }

// k, g (dk/da_e = -g (a_e - b_e)) and dk/dlog l of one pair: the policy's pair() (common.hpp), in the dtype.
// blockIdx.x = tile + tiles * slice.  A workgroup's scalar sums: [sum G k, sum G dk/dlog l], or with ARD
// [sum G k, sum G g df_0^2, .., sum G g df_{d-1}^2].
// The LIN arm's two more arguments: want_p says whether the partial P (ppart, laid out as dbpart) is written.  Without the
// arm the struct is empty, and the kernel is the one it was before the arm existed, instruction for instruction.
template <bool LIN> struct PairLin {};
template <> struct PairLin<true> { int want_p; double* ppart; };

template <typename T, int COV, int D, bool ARD, bool LIN = false>
__global__ __launch_bounds__(256)
void k_cov_pair_grad(const T* __restrict__ xa, int na, const T* __restrict__ xb, int nb, int d, const T* __restrict__ G, int64_t ldg,
                     T c, T sf2, int tiles, int slice_len, int want_db, double* __restrict__ dbpart, double* __restrict__ sumpart,
                     PairLin<LIN> pl)
{
    constexpr int EPL = 16 / (int)sizeof(T);    // elements per lane and row
    constexpr int LPR = PG_CT / EPL;            // lanes per tile row
    constexpr int RPI = 64 / LPR;               // rows per wave and load instruction
    constexpr int NPH = 4 * RPI;                // row phases of the workgroup
    constexpr int DD = D ? D : MAXD;
    constexpr int NS = ARD ? 1 + DD : 2;        // scalar sums of a lane
    __shared__ double red[NPH * PG_CT];
    __shared__ double sred[4][NS];
    const int slice = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - slice * tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cx = (lane % LPR) * EPL;          // first column of this lane inside the tile
    const int phase = wave * RPI + lane / LPR;
    const int gc = tile * PG_CT + cx;
    const int r0 = slice * slice_len, r1 = min(na, r0 + slice_len);

    T xc[EPL][DD];
#pragma unroll
    for (int b = 0; b < EPL; ++b)
#pragma unroll
        for (int k = 0; k < DD; ++k) xc[b][k] = ((D || k < d) && gc + b < nb) ? xb[(int64_t)(gc + b) * d + k] : (T)0;
    const bool whole = gc + EPL <= nb;          // the lane's chunk lies inside the matrix

    auto load_g = [&](int i, T* gv) {
        const T* src = G + (int64_t)i * ldg + gc;
        if (whole && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(src);
            __builtin_memcpy(gv, &v, 16);
        } else {
#pragma unroll
            for (int b = 0; b < EPL; ++b) gv[b] = (gc + b < nb) ? src[b] : (T)0;
        }
    };
    auto load_x = [&](int i, T* xr) {
#pragma unroll
        for (int k = 0; k < DD; ++k) xr[k] = (D || k < d) ? xa[(int64_t)i * d + k] : (T)0;
    };

    double acc[EPL][DD], sk = 0.0, sl = 0.0, sd[DD];    // sl: not ARD; sd: ARD
#pragma unroll
    for (int b = 0; b < EPL; ++b)
#pragma unroll
        for (int k = 0; k < DD; ++k) acc[b][k] = 0.0;
#pragma unroll
    for (int k = 0; k < DD; ++k) sd[k] = 0.0;
    double pacc[LIN ? EPL : 1][LIN ? DD : 1];           // LIN: sum_i G_ij xa_ie
    if constexpr (LIN) {
#pragma unroll
        for (int b = 0; b < EPL; ++b)
#pragma unroll
            for (int k = 0; k < DD; ++k) pacc[b][k] = 0.0;
    }

    T gcur[EPL], xcur[DD], gnext[EPL], xnext[DD];
    int i = r0 + phase;
    if (i < r1) { load_g(i, gcur); load_x(i, xcur); }
    for (; i < r1; i += NPH) {
        const bool more = i + NPH < r1;
        if (more) { load_g(i + NPH, gnext); load_x(i + NPH, xnext); }
#pragma unroll
        for (int b = 0; b < EPL; ++b) {
            T df[DD], d2 = (T)0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                df[k] = xcur[k] - xc[b][k];
                d2 += df[k] * df[k];
            }
            T kv, gv, lv;
            Cov<COV>::template pair<T, D>(d2, df[0], c, sf2, kv, gv, lv);
            const double w = (double)gcur[b];
            sk += w * (double)kv;
            if constexpr (!ARD) sl += w * (double)lv;
            const double wg = w * (double)gv;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                acc[b][k] += wg * (double)df[k];
                if constexpr (ARD) sd[k] += (wg * (double)df[k]) * (double)df[k];
                if constexpr (LIN) pacc[b][k] += w * (double)xcur[k];
            }
        }
        if (more) {
#pragma unroll
            for (int b = 0; b < EPL; ++b) gcur[b] = gnext[b];
#pragma unroll
            for (int k = 0; k < DD; ++k) xcur[k] = xnext[k];
        }
    }

    // the scalar sums: pairwise over the lanes of a wave (wave_sum, reduce.hpp), then the four waves in order (sum4)
    if constexpr (ARD) wave_sum(sk, sd);
    else               wave_sum(sk, sl);
    if (lane == 0) {
        sred[wave][0] = sk;
        if constexpr (!ARD) sred[wave][1] = sl;
        if constexpr (ARD) {
#pragma unroll
            for (int k = 0; k < DD; ++k) sred[wave][1 + k] = sd[k];
        }
    }
    __syncthreads();
    const int ns = ARD ? 1 + d : 2;             // the sums of the dimensions >= d (all 0) are not written
    if (tid < ns) sumpart[(int64_t)blockIdx.x * ns + tid] = sum4(sred[0][tid], sred[1][tid], sred[2][tid], sred[3][tid]);
    if constexpr (LIN) {
        // P: the same phase-order sum as db below, into ppart
        if (pl.want_p) {
            double* pout = pl.ppart + (int64_t)blockIdx.x * PG_CT * d;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (!(D || k < d)) break;
#pragma unroll
                for (int b = 0; b < EPL; ++b) red[phase * PG_CT + cx + b] = pacc[b][k];
                __syncthreads();
                if (tid < PG_CT) {
                    double s = red[tid];
#pragma unroll
                    for (int p = 1; p < NPH; ++p) s += red[p * PG_CT + tid];
                    pout[tid * d + k] = s;
                }
                __syncthreads();
            }
        }
    }
    if (!want_db) return;
    // db: per dimension, the NPH row phases of a column are added in phase order
    double* out = dbpart + (int64_t)blockIdx.x * PG_CT * d;
#pragma unroll
    for (int k = 0; k < DD; ++k) {
        if (!(D || k < d)) break;
#pragma unroll
        for (int b = 0; b < EPL; ++b) red[phase * PG_CT + cx + b] = acc[b][k];
        __syncthreads();
        if (tid < PG_CT) {
            double s = red[tid];
#pragma unroll
            for (int p = 1; p < NPH; ++p) s += red[p * PG_CT + tid];
            out[tid * d + k] = s;
        }
        __syncthreads();
    }
}

// blockIdx.x < dblocks: 256 elements of db, each the sum of its S partials in slice order; workgroup dblocks + c (sums
// wanted, c < nsums): thread t adds the partials t, t + 256, .. of scalar sum c (tile-major within a slice), then the 256
// partial sums are added pairwise in LDS (lds_tree, reduce.hpp).
// LIN: db gets scale (covariance part + lin_k P_jk), P_jk the sum of its S partials of ppart in slice order; workgroup
// dblocks + nsums_wg + k (k < d, lsums wanted; nsums_wg = nsums or 0 as the scalar sums are wanted): thread t adds
// xb_jk P_jk over j = t, t + 256, .., then lds_tree; lsums is not scaled.
template <typename T, bool LIN> struct ReduceLin {};
template <typename T> struct ReduceLin<T, true> { const double* ppart; const double* lin; const T* xb; int nsums_wg; double* lsums; };

template <typename T, bool LIN = false>
__global__ __launch_bounds__(256)
void k_pair_grad_reduce(const double* __restrict__ dbpart, const double* __restrict__ sumpart, int nb, int d, int tiles, int slices,
                        int dblocks, int nsums, double scale, int accumulate, T* __restrict__ db, double* __restrict__ sums,
                        ReduceLin<T, LIN> rl)
{
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < dblocks) {
        const int64_t e = (int64_t)blockIdx.x * 256 + tid;
        if (e >= (int64_t)nb * d) return;
        const int j = (int)(e / d), k = (int)(e - (int64_t)j * d);
        const int tile = j / PG_CT, jj = j - tile * PG_CT;
        const double* p = dbpart + ((int64_t)tile * PG_CT + jj) * d + k;
        double s = p[0];
        for (int sl = 1; sl < slices; ++sl) s += p[(int64_t)sl * tiles * PG_CT * d];
        if constexpr (LIN) {
            const double* pp = rl.ppart + ((int64_t)tile * PG_CT + jj) * d + k;
            double ps = pp[0];
            for (int sl = 1; sl < slices; ++sl) ps += pp[(int64_t)sl * tiles * PG_CT * d];
            s += rl.lin[k] * ps;
        }
        s *= scale;
        db[e] = accumulate ? (T)((double)db[e] + s) : (T)s;
        return;
    }
    __shared__ double red[256];
    const int c = (int)blockIdx.x - dblocks;
    if constexpr (LIN) {
        if (c >= rl.nsums_wg) {
            const int k = c - rl.nsums_wg;
            double s = 0.0;
            for (int j = tid; j < nb; j += 256) {
                const int tile = j / PG_CT, jj = j - tile * PG_CT;
                const double* pp = rl.ppart + ((int64_t)tile * PG_CT + jj) * d + k;
                double ps = pp[0];
                for (int sl = 1; sl < slices; ++sl) ps += pp[(int64_t)sl * tiles * PG_CT * d];
                s += (double)rl.xb[(int64_t)j * d + k] * ps;
            }
            red[tid] = s;
            lds_tree<256>(red, tid);
            if (tid == 0) rl.lsums[k] = accumulate ? rl.lsums[k] + red[0] : red[0];
            return;
        }
    }
    const int64_t parts = (int64_t)tiles * slices;
    double s = 0.0;
    for (int64_t p = tid; p < parts; p += 256) s += sumpart[nsums * p + c];
    red[tid] = s;
    lds_tree<256>(red, tid);
    if (tid == 0) sums[c] = accumulate ? sums[c] + red[0] : red[0];
}

// ----------------------------------------------------------------------- rows ----
// A wave per row (wave_row, reduce.hpp), as k_sparse_rowsq / k_sparse_tail: lane l takes columns l, l + 64, .. in FP64,
// then the 64 partial sums are added pairwise (wave_sum: xor 32, 16, .. 1): a fixed order.  t <- h_i (k_sparse_grad_sums
// turns it into t for VFE).
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_grad_rows(const T* __restrict__ V, int64_t ldv, int n, int m, const T* __restrict__ gamma, const T* __restrict__ r,
                        const T* __restrict__ w, int q, T* __restrict__ beta, T* __restrict__ t)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    const T* v = V + (int64_t)row * ldv;
    double sv = 0.0, acc[MAXQ] = {};
    for (int j = lane; j < m; j += 64) {
        const double vv = (double)v[j];
        sv += vv * vv;
        dot_step(acc, vv, gamma + (int64_t)j * q, q);
    }
    wave_sum(sv, acc);
    if (lane != 0) return;
    const double wi = (double)w[row];
    double bsq = 0.0;
#pragma unroll
    for (int c = 0; c < MAXQ; ++c) {
        if (c < q) {
            const double bt = wi * ((double)r[(int64_t)row * q + c] - acc[c]);
            beta[(int64_t)row * q + c] = (T)bt;
            bsq += bt * bt;
        }
    }
    t[row] = (T)(0.5 * (bsq - (double)q * (wi - wi * wi * sv)));
}

// One workgroup of 1024 threads: thread k takes i = k, k + 1024, ..; the 1024 partial sums are added pairwise in LDS
// (lds_tree).
template <typename T>
__global__ __launch_bounds__(1024)
void k_sparse_grad_sums(T* __restrict__ t, int n, int mode, double tvfe, double* __restrict__ sums)
{
    __shared__ double red[2][1024];
    const int tid = threadIdx.x;
    const T tv = (T)tvfe;
    double sh = 0.0, st = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const T h = t[i];
        sh += (double)h;
        if (mode == 1) {
            t[i] = tv;
            st += (double)tv;
        } else {
            st += (double)h;
        }
    }
    red[0][tid] = sh;
    red[1][tid] = st;
    lds_tree<1024, 2>(&red[0][0], tid);
    if (tid < 2) sums[tid] = red[tid][0];
}

// -------------------------------------------------------------------- combine ----
// A wave per row: lane l takes columns l, l + 64, ..: the loads and the store of a wave are contiguous runs.
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_grad_combine(const T* __restrict__ A, int64_t lda, T* __restrict__ Y, int64_t ldy, int n, int m,
                           const T* __restrict__ beta, const T* __restrict__ b, const T* __restrict__ w, const T* __restrict__ t, int q)
{
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double bt[MAXQ];
#pragma unroll
    for (int c = 0; c < MAXQ; ++c) bt[c] = c < q ? (double)beta[(int64_t)row * q + c] : 0.0;
    const double qw = (double)q * (double)w[row], t2 = 2.0 * (double)t[row];
    const T* a = A + (int64_t)row * lda;
    T* y = Y + (int64_t)row * ldy;
    for (int j = lane; j < m; j += 64) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < MAXQ; ++c)
            if (c < q) s += bt[c] * (double)b[(int64_t)j * q + c];
        y[j] = (T)(s - qw * (double)y[j] - t2 * (double)a[j]);
    }
}

}  // namespace

template <typename T, int COV, bool ARD>
static int pair_grad_run_cov(const T* xa, int64_t na, const T* xb, int64_t nb, int d, const T* g, int64_t ldg, double ell, double sf2,
                             double scale, int accumulate, double* sums, T* db, double* scratch, hipStream_t st, const char* fn)
{
    const int64_t tiles = pg_tiles(nb), len = pg_slice_len(na, nb), slices = pg_slices(na, nb);
    double* dbpart = scratch;
    double* sumpart = scratch + pg_dbpart_elems(na, nb, d);
    const dim3 grid((unsigned)(tiles * slices));
    const T c = (T)cov_scale(COV, ell);
    with_dim(d, [&](auto dd) {
        hipLaunchKernelGGL((k_cov_pair_grad<T, COV, decltype(dd)::value, ARD>), grid, dim3(256), 0, st, xa, (int)na, xb, (int)nb, d, g, ldg,
                           c, (T)sf2, (int)tiles, (int)len, db != nullptr ? 1 : 0, dbpart, sumpart, PairLin<false>());
    });
    CIMRGP_LAUNCH_CHECK(fn);
    const int64_t dblocks = db != nullptr ? (nb * d + 255) / 256 : 0;
    const int nsums = pg_nsums(d, ARD);
    hipLaunchKernelGGL((k_pair_grad_reduce<T>), dim3((unsigned)(dblocks + (sums != nullptr ? nsums : 0))), dim3(256), 0, st,
                       (const double*)dbpart, (const double*)sumpart, (int)nb, d, (int)tiles, (int)slices, (int)dblocks, nsums, scale,
                       accumulate, db, sums, ReduceLin<T, false>());
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

// The LIN arm: ppart lies behind the twin's two arrays.
template <typename T, int COV, bool ARD>
static int pair_grad_lin_run_cov(const T* xa, int64_t na, const T* xb, int64_t nb, int d, const T* g, int64_t ldg, double ell, double sf2,
                                 const double* lin, double scale, int accumulate, double* sums, double* lsums, T* db, double* scratch,
                                 hipStream_t st, const char* fn)
{
    const int64_t tiles = pg_tiles(nb), len = pg_slice_len(na, nb), slices = pg_slices(na, nb);
    const int nsums = pg_nsums(d, ARD);
    double* dbpart = scratch;
    double* sumpart = dbpart + pg_dbpart_elems(na, nb, d);
    double* ppart = sumpart + pg_sumpart_elems(na, nb, nsums);
    const dim3 grid((unsigned)(tiles * slices));
    const T c = (T)cov_scale(COV, ell);
    with_dim(d, [&](auto dd) {
        hipLaunchKernelGGL((k_cov_pair_grad<T, COV, decltype(dd)::value, ARD, true>), grid, dim3(256), 0, st, xa, (int)na, xb, (int)nb, d,
                           g, ldg, c, (T)sf2, (int)tiles, (int)len, db != nullptr ? 1 : 0, dbpart, sumpart,
                           PairLin<true>{(db != nullptr || lsums != nullptr) ? 1 : 0, ppart});
    });
    CIMRGP_LAUNCH_CHECK(fn);
    const int64_t dblocks = db != nullptr ? (nb * d + 255) / 256 : 0;
    const int nsums_wg = sums != nullptr ? nsums : 0;
    hipLaunchKernelGGL((k_pair_grad_reduce<T, true>), dim3((unsigned)(dblocks + nsums_wg + (lsums != nullptr ? d : 0))), dim3(256), 0, st,
                       (const double*)dbpart, (const double*)sumpart, (int)nb, d, (int)tiles, (int)slices, (int)dblocks, nsums, scale,
                       accumulate, db, sums, ReduceLin<T, true>{(const double*)ppart, lin, xb, nsums_wg, lsums});
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

static size_t pair_grad_scratch_bytes(int64_t na, int64_t nb, int d, bool ard)
{
    if (!pg_sizes_ok(na, nb, d)) return 0;
    return (size_t)(pg_dbpart_elems(na, nb, d) + pg_sumpart_elems(na, nb, pg_nsums(d, ard))) * sizeof(double);
}

static size_t pair_grad_lin_scratch_bytes(int64_t na, int64_t nb, int d, bool ard)
{
    if (!pg_sizes_ok(na, nb, d)) return 0;
    return pair_grad_scratch_bytes(na, nb, d, ard) + (size_t)pg_dbpart_elems(na, nb, d) * sizeof(double);
}

// The entry point of the contractions: `ard` selects the arm (sums_dev: 2 or 1 + d doubles), fn names it in errors.
// lin_entry: cimrgp_cov_pair_grad_lin, with its weights lin_dev (required) and lsums_dev (d doubles, may be NULL).
static int pair_grad_entry(const char* fn, bool ard, int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb,
                           int d, const void* g_dev, int64_t ldg, double ell, double sf2, double scale, int accumulate, double* sums_dev,
                           void* db_dev, void* scratch_dev, size_t scratch_bytes, void* stream, bool lin_entry = false,
                           const double* lin_dev = nullptr, double* lsums_dev = nullptr)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(xa_dev && xb_dev && g_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(!lin_entry || lin_dev, fn, "null pointer (lin)");
    CIMRGP_REQUIRE(na >= 1 && na <= CIMRGP_PAIR_GRAD_MAX_NA, fn, "na must be in [1, 16777216]");
    CIMRGP_REQUIRE(nb >= 1 && nb <= CIMRGP_PAIR_GRAD_MAX_NB, fn, "nb must be in [1, 1048576]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ldg >= nb, fn, "leading dimension too small");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    CIMRGP_REQUIRE((reinterpret_cast<uintptr_t>(scratch_dev) & 7u) == 0, fn, "scratch must be 8-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= (lin_entry ? pair_grad_lin_scratch_bytes(na, nb, d, ard) : pair_grad_scratch_bytes(na, nb, d, ard)), fn,
                   "scratch too small");
    if (sums_dev == nullptr && db_dev == nullptr && lsums_dev == nullptr) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return with_cov(cov, [&](auto cv) {
            constexpr int COV = decltype(cv)::value;
            if (lin_entry) {
                auto run = ard ? pair_grad_lin_run_cov<T, COV, true> : pair_grad_lin_run_cov<T, COV, false>;
                return run((const T*)xa_dev, na, (const T*)xb_dev, nb, d, (const T*)g_dev, ldg, ell, sf2, lin_dev, scale, accumulate,
                           sums_dev, lsums_dev, (T*)db_dev, (double*)scratch_dev, stream_of(stream), fn);
            }
            auto run = ard ? pair_grad_run_cov<T, COV, true> : pair_grad_run_cov<T, COV, false>;
            return run((const T*)xa_dev, na, (const T*)xb_dev, nb, d, (const T*)g_dev, ldg, ell, sf2, scale, accumulate, sums_dev,
                       (T*)db_dev, (double*)scratch_dev, stream_of(stream), fn);
        });
    });
}

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

size_t cimrgp_cov_pair_grad_scratch_bytes(int64_t na, int64_t nb, int d) { return pair_grad_scratch_bytes(na, nb, d, false); }

int cimrgp_cov_pair_grad(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, const void* g_dev,
                         int64_t ldg, double ell, double sf2, double scale, int accumulate, double* sums_dev, void* db_dev,
                         void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return pair_grad_entry("cimrgp_cov_pair_grad", false, dtype, cov, xa_dev, na, xb_dev, nb, d, g_dev, ldg, ell, sf2, scale, accumulate,
                           sums_dev, db_dev, scratch_dev, scratch_bytes, stream);
}

size_t cimrgp_cov_pair_grad_ard_scratch_bytes(int64_t na, int64_t nb, int d) { return pair_grad_scratch_bytes(na, nb, d, true); }

int cimrgp_cov_pair_grad_ard(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, const void* g_dev,
                             int64_t ldg, double ell, double sf2, double scale, int accumulate, double* sums_dev, void* db_dev,
                             void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return pair_grad_entry("cimrgp_cov_pair_grad_ard", true, dtype, cov, xa_dev, na, xb_dev, nb, d, g_dev, ldg, ell, sf2, scale, accumulate,
                           sums_dev, db_dev, scratch_dev, scratch_bytes, stream);
}

size_t cimrgp_cov_pair_grad_lin_scratch_bytes(int64_t na, int64_t nb, int d, int ard)
{
    return pair_grad_lin_scratch_bytes(na, nb, d, ard != 0);
}

int cimrgp_cov_pair_grad_lin(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, const void* g_dev,
                             int64_t ldg, double ell, double sf2, int ard, const double* lin_dev, double scale, int accumulate,
                             double* sums_dev, double* lsums_dev, void* db_dev, void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return pair_grad_entry("cimrgp_cov_pair_grad_lin", ard != 0, dtype, cov, xa_dev, na, xb_dev, nb, d, g_dev, ldg, ell, sf2, scale,
                           accumulate, sums_dev, db_dev, scratch_dev, scratch_bytes, stream, true, lin_dev, lsums_dev);
}

int cimrgp_sparse_grad_rows(int dtype, const void* v_dev, int64_t n, int64_t m, int64_t ldv, const void* gamma_dev, const void* r_dev,
                            const void* w_dev, int q, int mode, double noise, void* beta_dev, void* t_dev, double* sums_dev, void* stream)
{
    const char* fn = "cimrgp_sparse_grad_rows";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(v_dev && gamma_dev && r_dev && w_dev && beta_dev && t_dev && sums_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 31) && m >= 1 && m < (1ll << 31) && ldv >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(mode == 0 || mode == 1, fn, "mode must be 0 (FITC) or 1 (VFE)");
    CIMRGP_REQUIRE(noise > 0.0, fn, "noise must be positive");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_grad_rows<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)v_dev, ldv,
                           (int)n, (int)m, (const T*)gamma_dev, (const T*)r_dev, (const T*)w_dev, q, (T*)beta_dev, (T*)t_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL((k_sparse_grad_sums<T>), dim3(1), dim3(1024), 0, stream_of(stream), (T*)t_dev, (int)n, mode,
                           -0.5 * (double)q / noise, sums_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

int cimrgp_sparse_grad_combine(int dtype, const void* a_dev, int64_t lda, void* y_dev, int64_t ldy, int64_t n, int64_t m,
                               const void* beta_dev, const void* b_dev, const void* w_dev, const void* t_dev, int q, void* stream)
{
    const char* fn = "cimrgp_sparse_grad_combine";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(a_dev && y_dev && beta_dev && b_dev && w_dev && t_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 31) && m >= 1 && m < (1ll << 31) && lda >= m && ldy >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_grad_combine<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)a_dev, lda,
                           (T*)y_dev, ldy, (int)n, (int)m, (const T*)beta_dev, (const T*)b_dev, (const T*)w_dev, (const T*)t_dev, q);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

}  // extern "C"
