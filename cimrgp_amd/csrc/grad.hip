// Derivatives of the dense block posterior with respect to the test inputs (include/cimrgp_grad.h):
//   trsm_rows_lt   B <- B L^-1, panels of 256 columns from the last to the first:
//                    k_rows_lt_diag     B_p <- B_p inv(L_pp)   (a 16-row strip of the panel in LDS, in place; the inverse
//                                       is the (L_pp^-1)^T block the factorisation left in its workspace)
//                    k_rows_lt_update   B_{<p} -= B_p L[p, <p] (64 x 64 tiles; L[p, <p] is a row block of the row-major
//                                       factor, an A B product: its operand is staged into LDS transposed)
//                  both on the matrix cores (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Mx<T> in common.hpp)
//   predict_grad   k_cov_predict_grad: g(r) recomputed per (test point, training point) pair, both contractions in one
//                  pass over the pairs; the cross-covariance and its derivative are never stored
//   layer_grad     per block: the shared cross-Gram and forward row solve (cross_solve_run, layer.hip), the batched
//                  backward row solve above, then the batched contraction
#include "abi.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

// ---------------------------------------------------------------- B_p <- B_p inv(L_pp) ----
// One workgroup = 16 rows of B and the whole panel (w <= 256 columns): the strip is read into LDS before anything is
// written, so the product can go back in place.  Wave v owns output columns [64 v, 64 v + 64) (four 16 x 16 tiles).
// inv(L_pp)[k][j] = invT[j][k]: the right operand's fragment (B^T[col][kslot]) is a row segment of invT, read straight
// from global memory (the 256 x 256 block is shared by every strip and stays in the caches).
template <typename T>
__global__ __launch_bounds__(256)
void k_rows_lt_diag(T* __restrict__ B, int64_t ldb, int m, int c0, int w, const T* __restrict__ invT, int64_t sb, int64_t sws)
{
    using X = Mx<T>;
    using acc_t = typename X::acc_t;
    constexpr int LDS_LD = CIMRGP_NB + 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T strip[16 * LDS_LD];
    B += (int64_t)blockIdx.y * sb;
    invT += (int64_t)blockIdx.y * sws;
    const int r0 = (int)blockIdx.x * 16;
    const int mrows = min(16, m - r0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < 16 * CIMRGP_NB; e += 256) {
        const int r = e >> 8, c = e & (CIMRGP_NB - 1);
        strip[r * LDS_LD + c] = (r < mrows && c < w) ? B[(int64_t)(r0 + r) * ldb + c0 + c] : (T)0;
    }
    __syncthreads();
    const int j0 = wave * 64;
    if (j0 >= w) return;
    acc_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = acc_zero<T>();
    const int frow = lane & 15, fslot = lane >> 4;
    constexpr int KSTEP = 4 * X::EPS;
    for (int k0 = 0; k0 < w; k0 += KSTEP) {
        const int kk = k0 + fslot * X::EPS;
        const uint2 a = *reinterpret_cast<const uint2*>(&strip[frow * LDS_LD + kk]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = j0 + 16 * t + frow;
            T bv[2] = {(T)0, (T)0};
            if (col < w) {
                const T* src = invT + (int64_t)col * CIMRGP_NB + kk;
#pragma unroll
                for (int e = 0; e < X::EPS; ++e) bv[e] = (kk + e < w) ? src[e] : (T)0;
            }
            uint2 b;
            if constexpr (sizeof(T) == 8) {
                b = *reinterpret_cast<const uint2*>(&bv[0]);
            } else {
                b.x = __float_as_uint((float)bv[0]);
                b.y = __float_as_uint((float)bv[1]);
            }
            acc[t] = X::mma(a, b, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = j0 + 16 * t + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = X::crow(lane, r);
            if (row < mrows && col < w) B[(int64_t)(r0 + row) * ldb + c0 + col] = acc[t][r];
        }
    }
}

// ------------------------------------------------------------- B_{<p} -= B_p L[p, <p] ----
// C (m x N) -= A (m x K) Lb (K x N): C = columns [0, c0) of B, A = the panel's columns [c0, c0 + w), Lb = rows
// [c0, c0 + w) of L, columns [0, c0) (N = c0 is a multiple of 256, so column tiles are never ragged).  64 x 64 tiles,
// four waves in 2 x 2, each 32 x 32 = 2 x 2 MFMA tiles; K in stages of 32 through LDS.  Lb's stage (32 rows of 64
// contiguous elements) is stored transposed, so that both operands' fragments are 8-byte LDS reads of one row.
constexpr int UP_T = 64;
constexpr int UP_K = 32;

template <typename T>
__global__ __launch_bounds__(256)
void k_rows_lt_update(T* __restrict__ B, int64_t ldb, int m, int c0, int w, const T* __restrict__ L, int64_t ldl, int tiles_m,
                      int64_t sb, int64_t sl)
{
    using X = Mx<T>;
    using acc_t = typename X::acc_t;
    constexpr int LD = UP_K + 8 / (int)sizeof(T) * 2;   // 8-byte aligned rows, offset against bank conflicts
    __shared__ __attribute__((aligned(16))) T As[UP_T * LD];
    __shared__ __attribute__((aligned(16))) T Bs[UP_T * LD];
    B += (int64_t)blockIdx.y * sb;
    L += (int64_t)blockIdx.y * sl;
    const int id = blockIdx.x;
    const int tj = id / tiles_m, ti = id - tj * tiles_m;
    const int row0 = ti * UP_T, col0 = tj * UP_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const T* A = B + c0;                               // the panel's columns
    const T* Lb = L + (int64_t)c0 * ldl;               // the panel's rows of L
    acc_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = acc_zero<T>();
    const int frow = lane & 15, fslot = lane >> 4;
    // staging maps: A: row tid / 4, 8 consecutive k;  Lb: k row tid / 8, 8 consecutive columns
    const int ar = tid >> 2, ak = (tid & 3) * 8;
    const int bk = tid >> 3, bn = (tid & 7) * 8;
    const bool a_row_ok = row0 + ar < m;
    for (int k0 = 0; k0 < w; k0 += UP_K) {
        T va[8], vb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + ak + e;
            va[e] = (a_row_ok && k < w) ? A[(int64_t)(row0 + ar) * ldb + k] : (T)0;
        }
        const bool b_ok = k0 + bk < w;
#pragma unroll
        for (int e = 0; e < 8; ++e) vb[e] = b_ok ? Lb[(int64_t)(k0 + bk) * ldl + col0 + bn + e] : (T)0;
        __syncthreads();                               // the previous stage's fragments have been read
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            As[ar * LD + ak + e] = va[e];
            Bs[(bn + e) * LD + bk] = vb[e];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < UP_K; ks += 4 * X::EPS) {
            const int kk = ks + fslot * X::EPS;
            uint2 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const uint2*>(&As[(wr * 32 + i * 16 + frow) * LD + kk]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const uint2*>(&Bs[(wc * 32 + j * 16 + frow) * LD + kk]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = X::mma(a[i], b[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gc = col0 + wc * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gr = row0 + wr * 32 + i * 16 + X::crow(lane, r);
                if (gr < m) {
                    T* p = B + (int64_t)gr * ldb + gc;
                    *p = *p - acc[i][j][r];
                }
            }
        }
}

// ------------------------------------------------------------------- the contraction ----
// dk/dx*_e = -g (x*_e - x_e), g of the policy's pair() (common.hpp; c is the policy's scale, cov_scale).  256 threads = 8 test points x 32 phases (32 consecutive lanes per test point: their beta reads are one contiguous
// 32-element segment of the row, and the reduction over the phases stays inside half a wave -- shuffles, no LDS).
// blockIdx.y = block of a batch (starts / t_starts NULL: one block at offset 0).
constexpr int PG_TS = 8;
constexpr int PG_PH = 32;

template <typename T, int COV, int D, int Q>
__global__ __launch_bounds__(256)
void k_cov_predict_grad(const T* __restrict__ x, const int64_t* __restrict__ starts, int n, int d, const T* __restrict__ alpha,
                        int64_t sa, int q, const T* __restrict__ xs, const int64_t* __restrict__ t_starts, int ns, T c, T sf2,
                        const T* __restrict__ beta, int64_t ldb, int64_t sbeta, T* __restrict__ mg, T* __restrict__ vg,
                        int accumulate)
{
    constexpr int DD = D ? D : MAXD;
    const int64_t b = blockIdx.y;
    const int64_t xoff = starts ? starts[b] : 0;
    const int64_t toff = t_starts ? t_starts[b] : 0;
    x += xoff * d;
    alpha += b * sa;
    if (beta) beta += b * sbeta;
    const int tid = threadIdx.x;
    const int ph = tid & (PG_PH - 1);
    const int gi = (int)blockIdx.x * PG_TS + tid / PG_PH;
    const bool valid = gi < ns;
    const bool want_mean = mg != nullptr, want_var = vg != nullptr;
    T xt[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) xt[k] = ((D || k < d) && valid) ? xs[(toff + gi) * d + k] : (T)0;
    T ms[DD][Q], vs[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) {
        vs[k] = (T)0;
#pragma unroll
        for (int cc = 0; cc < Q; ++cc) ms[k][cc] = (T)0;
    }
    const T* brow = want_var && valid ? beta + (int64_t)gi * ldb : nullptr;
    const int nloop = valid ? n : 0;
    for (int j = ph; j < nloop; j += PG_PH) {
        T df[DD];
        T d2 = (T)0;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            df[k] = (D || k < d) ? xt[k] - x[(int64_t)j * d + k] : (T)0;
            d2 += df[k] * df[k];
        }
        T kv, g, lv;
        Cov<COV>::template pair<T, D>(d2, df[0], c, sf2, kv, g, lv);
        if (want_mean) {
#pragma unroll
            for (int cc = 0; cc < Q; ++cc) {
                if (cc < q) {
                    const T ga = g * alpha[(int64_t)j * q + cc];
#pragma unroll
                    for (int k = 0; k < DD; ++k) ms[k][cc] -= ga * df[k];
                }
            }
        }
        if (want_var) {
            const T gb = g * brow[j];
#pragma unroll
            for (int k = 0; k < DD; ++k) vs[k] += gb * df[k];
        }
    }
    // sum over the 32 phases of this test point (lanes ph = 0..31 of one half wave): wave_sum over 32 lanes
    // (reduce.hpp)
    wave_sum<PG_PH>(vs, ms);
    if (ph != 0 || !valid) return;
    const int64_t row = toff + gi;
    if (want_mean) {
        T* o = mg + row * d * q;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (!(D || k < d)) continue;
#pragma unroll
            for (int cc = 0; cc < Q; ++cc) {
                if (cc < q) o[k * q + cc] = accumulate ? o[k * q + cc] + ms[k][cc] : ms[k][cc];
            }
        }
    }
    if (want_var) {
        T* o = vg + row * d;
#pragma unroll
        for (int k = 0; k < DD; ++k) {
            if (!(D || k < d)) continue;
            const T v = (T)2 * vs[k];
            o[k] = accumulate ? o[k] + v : v;
        }
    }
}

}  // namespace

// B <- B L^-1 for bt.count blocks (strides bt.sk of L, bt.sws of the workspace, bt.sb of B, in elements)
template <typename T>
static int rows_lt_run(const T* l, int64_t n, int64_t ldl, const T* ws, T* b, int64_t m, int64_t ldb, hipStream_t st, PotrfBatch bt,
                       const char* fn)
{
    if (n <= 0 || m <= 0) return 0;
    const int64_t npan = (n + CIMRGP_NB - 1) / CIMRGP_NB;
    const T* invT = ws + ws_invT_offset(n);
    const int64_t strips = (m + 15) / 16, tiles_m = (m + UP_T - 1) / UP_T;
    CIMRGP_REQUIRE(strips < (1ll << 31) && tiles_m * (n / UP_T + 1) < (1ll << 31), fn, "grid too large");
    for (int64_t p = npan - 1; p >= 0; --p) {
        const int64_t c0 = p * CIMRGP_NB;
        const int w = (int)std::min<int64_t>(CIMRGP_NB, n - c0);
        hipLaunchKernelGGL((k_rows_lt_diag<T>), dim3((unsigned)strips, (unsigned)bt.count), dim3(256), 0, st, b, ldb, (int)m, (int)c0, w,
                           invT + p * (CIMRGP_NB * CIMRGP_NB), bt.sb, bt.sws);
        CIMRGP_LAUNCH_CHECK(fn);
        if (c0 == 0) continue;
        const int64_t tiles = tiles_m * (c0 / UP_T);
        hipLaunchKernelGGL((k_rows_lt_update<T>), dim3((unsigned)tiles, (unsigned)bt.count), dim3(256), 0, st, b, ldb, (int)m, (int)c0,
                           w, l, ldl, (int)tiles_m, bt.sb, bt.sk);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    return 0;
}

// the contraction of a.bc.batch blocks; beta: a.w's arena with the rows of K(xs, x) K^-1, or NULL (no variance gradient)
template <typename T, int COV>
static int predict_grad_run_cov(const LayerGrad<T>& a, const T* beta, hipStream_t st, const char* fn)
{
    if (a.te.n <= 0 || (a.mg == nullptr && a.vg == nullptr)) return 0;
    const dim3 grid((unsigned)((a.te.n + PG_TS - 1) / PG_TS), (unsigned)a.bc.batch);
    const T c = (T)cov_scale(COV, a.bc.ell);
    with_q_rounded(a.q, [&](auto qq) {            // 5 .. 8: the run-time guard c < q
        with_dim(a.bc.d, [&](auto dd) {
            hipLaunchKernelGGL((k_cov_predict_grad<T, COV, decltype(dd)::value, decltype(qq)::value>), grid, dim3(256), 0, st, a.tr.x,
                               a.tr.starts, (int)a.tr.n, a.bc.d, a.alpha, a.sa, a.q, a.te.x, a.te.starts, (int)a.te.n, c, (T)a.bc.sf2, beta,
                               a.w.ld, a.w.stride, a.mg, a.vg, a.accumulate);
        });
    });
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
static int predict_grad_run(const LayerGrad<T>& a, const T* beta, hipStream_t st, const char* fn)
{
    return with_cov(a.bc.cov, [&](auto cv) { return predict_grad_run_cov<T, decltype(cv)::value>(a, beta, st, fn); });
}

template <typename T>
static int layer_grad_run(const LayerGrad<T>& a, hipStream_t st)
{
    const char* fn = "cimrgp_layer_predict_grad_cov";
    if (a.te.n <= 0 || (a.mg == nullptr && a.vg == nullptr)) return 0;
    if (a.vg != nullptr) {
        // W_b = K(xs_b, x_b) L_b^-T, then beta_b = W_b L_b^-1
        int rc = cross_solve_run<T>(a.bc, a.tr, a.f, a.te, a.w, st);
        if (rc) return rc;
        rc = rows_lt_run<T>(a.f.l.p, a.tr.n, a.f.l.ld, a.f.ws, a.w.p, a.te.n, a.w.ld, st, potrf_batch(a.bc.batch, a.f, a.w.stride), fn);
        if (rc) return rc;
    }
    return predict_grad_run<T>(a, a.vg ? (const T*)a.w.p : nullptr, st, fn);
}

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_trsm_rows_lt_batched(int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride, const void* workspace_dev,
                                size_t workspace_stride_bytes, void* b_dev, int64_t m, int64_t ldb, int64_t b_stride, int batch,
                                void* stream)
{
    const char* fn = "cimrgp_trsm_rows_lt";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(l_dev && workspace_dev && b_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 30) && m >= 0 && m < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(ldl >= n && ldb >= n, fn, "leading dimension too small");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldb % e == 0 && l_stride % e == 0 && b_stride % e == 0, fn,
                   "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(l_dev) && aligned16(workspace_dev) && aligned16(b_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n) || batch == 1, fn, "workspace stride too small");
    CIMRGP_REQUIRE(workspace_stride_bytes % 16 == 0 || batch == 1, fn, "workspace stride must be a multiple of 16 bytes");
    CIMRGP_REQUIRE(batch == 1 || m == 0 || b_stride >= (m - 1) * ldb + n, fn, "block stride too small");
    const PotrfBatch bt{batch, l_stride, (int64_t)(workspace_stride_bytes / elem_bytes(dtype)), b_stride};
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return rows_lt_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)b_dev, m, ldb, stream_of(stream), bt, fn);
    });
}

int cimrgp_trsm_rows_lt(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* b_dev, int64_t m,
                        int64_t ldb, void* stream)
{
    return cimrgp_trsm_rows_lt_batched(dtype, l_dev, n, ldl, 0, workspace_dev, 0, b_dev, m, ldb, 0, 1, stream);
}

int cimrgp_cov_predict_grad(int dtype, int cov, const void* x_dev, int64_t n, int d, const void* alpha_dev, int q, const void* xs_dev,
                            int64_t ns, double ell, double sf2, const void* beta_dev, int64_t ldb, void* mean_grad_dev,
                            void* var_grad_dev, int accumulate, void* stream)
{
    const char* fn = "cimrgp_cov_predict_grad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(x_dev && xs_dev, fn, "null pointer");
    CIMRGP_REQUIRE(mean_grad_dev == nullptr || alpha_dev != nullptr, fn, "null pointer (alpha)");
    CIMRGP_REQUIRE(var_grad_dev == nullptr || beta_dev != nullptr, fn, "null pointer (beta)");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 31) && ns >= 0 && ns < (1ll << 31), fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    CIMRGP_REQUIRE(var_grad_dev == nullptr || ldb >= n, fn, "leading dimension of beta smaller than n");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerGrad<T> a;
        a.bc = BatchCov{1, d, cov, ell, sf2};
        a.tr = Points<T>{(const T*)x_dev, nullptr, n};
        a.te = Points<T>{(const T*)xs_dev, nullptr, ns};
        a.alpha = (const T*)alpha_dev; a.q = q;
        a.w.ld = ldb;
        a.mg = (T*)mean_grad_dev; a.vg = (T*)var_grad_dev; a.accumulate = accumulate;
        return predict_grad_run<T>(a, (const T*)beta_dev, stream_of(stream), fn);
    });
}

int cimrgp_layer_predict_grad_cov(int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d, const void* xs_dev,
                                  const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2, const void* l_arena_dev,
                                  int64_t ldl, int64_t l_stride, const void* ws_arena_dev, size_t ws_stride_bytes, const void* alpha_dev,
                                  int q, void* w_arena_dev, int64_t ldw, int64_t w_stride, void* mean_grad_dev, void* var_grad_dev,
                                  int accumulate, void* stream)
{
    const char* fn = "cimrgp_layer_predict_grad_cov";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(x_dev && starts_dev && xs_dev && t_starts_dev && alpha_dev, fn, "null pointer");
    CIMRGP_REQUIRE(var_grad_dev == nullptr || (l_arena_dev && ws_arena_dev && w_arena_dev), fn, "null pointer (factor, workspace or W)");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 30) && ns >= 0 && ns < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    if (var_grad_dev != nullptr) {
        CIMRGP_REQUIRE(ldl >= n && ldw >= n, fn, "leading dimension too small");
        const int64_t e = elems_per_16_bytes(dtype);
        CIMRGP_REQUIRE(ldl % e == 0 && ldw % e == 0 && l_stride % e == 0 && w_stride % e == 0, fn,
                       "leading dimensions and strides must be multiples of 16 bytes");
        CIMRGP_REQUIRE(aligned16(l_arena_dev) && aligned16(ws_arena_dev) && aligned16(w_arena_dev), fn, "pointers must be 16-byte aligned");
        CIMRGP_REQUIRE(ws_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n) || batch == 1, fn, "workspace stride too small");
        CIMRGP_REQUIRE(ws_stride_bytes % 16 == 0 || batch == 1, fn, "workspace stride must be a multiple of 16 bytes");
        CIMRGP_REQUIRE(batch == 1 || ns == 0 || (block_stride_ok(l_stride, n, n, ldl) && w_stride >= (ns - 1) * ldw + n), fn,
                       "block stride too small");
    }
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerGrad<T> a;
        a.bc = BatchCov{batch, d, cov, ell, sf2};
        a.tr = Points<T>{(const T*)x_dev, starts_dev, n};
        a.te = Points<T>{(const T*)xs_dev, t_starts_dev, ns};
        a.f = Factors<const T>{{(const T*)l_arena_dev, ldl, l_stride}, (const T*)ws_arena_dev, (int64_t)(ws_stride_bytes / sizeof(T))};
        a.alpha = (const T*)alpha_dev; a.sa = n * q; a.q = q;
        a.w = Arena<T>{(T*)w_arena_dev, ldw, w_stride};
        a.mg = (T*)mean_grad_dev; a.vg = (T*)var_grad_dev; a.accumulate = accumulate;
        return layer_grad_run<T>(a, stream_of(stream));
    });
}

}  // extern "C"
