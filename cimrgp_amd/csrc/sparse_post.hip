// Posterior queries of the sparse (inducing-point) GP: the four calls of include/cimrgp_sparse_post.h.
//   cov_cross_grad    k_cov_cross_grad    one 64 x 64 tile of the pairs (xa_i, xb_j) per workgroup: k and g from ONE
//                                         exponential per pair (k_and_g), written as d + 1 slabs (k, then
//                                         -g (xa_e - xb_e) per e)
//   sparse_tail_grad  k_sparse_tail_grad  a wave per (test row, dimension): dW_e gamma and 2 (W* . dW_e - A* . dA_e)
//   sparse_loo        k_sparse_loo        a wave per training row: q_i, lambda_i, h_i, V_i gamma -> LOO mean and variance
//   sparse_joint_cov  the Gram tiles (gram.hip), C -= A* A*^T (gemm_nt_sub as a SYRK), C += W* W*^T (k_syrk_add_lower:
//                     gemm_tile's body, LOWER and ADD), optionally the factorisation and a zeroed strict upper triangle
//
// k_cov_cross_grad.  The lane layout is the cross-Gram kernel's (gram.hip, gram_lanes): a lane owns the 16 bytes of a
// row it stores with one instruction -- EPL = 2 doubles / 4 floats -- and the lanes of a wave are adjacent along the
// row, so every store instruction writes whole 512-byte runs of every slab.  The arithmetic of slab 0 is gram_lanes'
// own, expression for expression (the differences, their squares added in dimension order, the policy's value), so the
// slab is bit-identical to cimrgp_cov_cross's output.  The lane's EPL points of xb stay in registers; the row's point of
// xa is one address for all lanes of the row.  No LDS: nothing is handed from wave to wave.
// The row kernels follow k_sparse_tail (sparse.hip): lane l takes columns l, l + 64, .. in FP64, then the 64 partial sums
// are added pairwise (xor 32, 16, .. 1) -- a fixed order that depends on m alone.
#include "abi.hpp"
#include "reduce.hpp"
#include "gemm_tile.hpp"

namespace cimrgp {

namespace {

constexpr int CG_TILE = 64;

// k and g of one pair from ONE exponential.  k is the policy's value(), the call the Gram kernels make, and the two empty
// assembly statements fence it: nothing of g's arithmetic is shared with it, so k's instructions are those of gram.hip and
// slab 0 is bit-identical to cimrgp_cov_cross's output.  (Cov<COV>::pair, which shares t, 1 + t and exp(-t) between k
// and g, gave a Matern 5/2 k one or two FP32 roundings off value()'s: the shared terms change which products hipcc
// contracts.)  g then follows from k by a division instead of a second exponential:
//   RBF k / l^2 | Matern 1/2 k c / r (0 at r = 0) | 3/2 c^2 k / (1 + t) | 5/2 c^2 k (1 + t) / (3 (1 + t + t^2 / 3)),  t = c r.
template <int COV, typename T, int D>
static __device__ __forceinline__ void k_and_g(T d2, T df0, T c, T sf2, T& k, T& g)
{
    k = Cov<COV>::template value<T, D>(d2, df0, c, sf2);
    asm volatile("" : "+v"(k));
    if constexpr (COV == CIMRGP_COV_RBF) {
        g = k * ((T)-2 * c);
    } else {
        T d2b = d2, dfb = df0;
        asm volatile("" : "+v"(d2b), "+v"(dfb));
        const T r = MaternCov<COV>::template radius<T, D>(d2b, dfb);
        const T t = c * r;
        if constexpr (COV == CIMRGP_COV_MATERN12) g = r > (T)0 ? k * c / r : (T)0;
        else if constexpr (COV == CIMRGP_COV_MATERN32) g = c * c * k / ((T)1 + t);
        else g = c * c * k * ((T)1 + t) * (T)(1.0 / 3.0) / MaternCov<COV>::poly(t);
    }
}

template <typename T, int COV, int D>
__global__ __launch_bounds__(256)
void k_cov_cross_grad(const T* __restrict__ xa, int na, const T* __restrict__ xb, int nb, int d, T c, T sf2, T* __restrict__ out,
                      int64_t ldo, int64_t ss, int tiles_n)
{
    constexpr int EPL = 16 / (int)sizeof(T);    // elements per lane and row
    constexpr int LPR = CG_TILE / EPL;          // lanes per tile row
    constexpr int RPI = 64 / LPR;               // rows per wave and store instruction
    constexpr int NIT = CG_TILE / (4 * RPI);    // row iterations: 4 waves x RPI rows each
    constexpr int DD = D ? D : MAXD;
    const int ti = (int)blockIdx.x / tiles_n, tj = (int)blockIdx.x - ti * tiles_n;
    const int row0 = ti * CG_TILE, col0 = tj * CG_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cx = (lane % LPR) * EPL, ry = lane / LPR;
    const int gc = col0 + cx;
    if (gc >= nb) return;
    T xc[EPL][DD];
#pragma unroll
    for (int b = 0; b < EPL; ++b)
#pragma unroll
        for (int k = 0; k < DD; ++k) xc[b][k] = ((D || k < d) && gc + b < nb) ? xb[(int64_t)(gc + b) * d + k] : (T)0;
    const bool whole = gc + EPL <= nb;

#pragma unroll
    for (int a = 0; a < NIT; ++a) {
        const int gr = row0 + (a * 4 + wave) * RPI + ry;
        if (gr >= na) continue;
        T xr[DD];
#pragma unroll
        for (int k = 0; k < DD; ++k) xr[k] = (D || k < d) ? xa[(int64_t)gr * d + k] : (T)0;
        T o[DD + 1][EPL];
#pragma unroll
        for (int b = 0; b < EPL; ++b) {
            T dfv[DD], d2 = (T)0, df0 = (T)0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                dfv[k] = (T)0;
                if (D || k < d) {
                    const T df = xr[k] - xc[b][k];
                    if (COV != CIMRGP_COV_RBF && k == 0) df0 = df;
                    d2 += df * df;
                    dfv[k] = df;
                }
            }
            T kv, gv;
            k_and_g<COV, T, D>(d2, df0, c, sf2, kv, gv);
            o[0][b] = kv;
#pragma unroll
            for (int k = 0; k < DD; ++k) o[1 + k][b] = -(gv * dfv[k]);
        }
#pragma unroll
        for (int s = 0; s < DD + 1; ++s) {
            if (!(D || s <= d)) continue;
            T* dst = out + (int64_t)s * ss + (int64_t)gr * ldo + gc;
            if (whole && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                uint4 v;
                __builtin_memcpy(&v, o[s], 16);
                *reinterpret_cast<uint4*>(dst) = v;
            } else {
#pragma unroll
                for (int b = 0; b < EPL; ++b)
                    if (gc + b < nb) dst[b] = o[s][b];
            }
        }
    }
}

// A wave per (row, e), 4 per workgroup (wave_row, reduce.hpp); the lanes' partial sums are added by wave_sum.  A, gamma,
// mg, vg may be nullptr as the entry point allows.
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_tail_grad(const T* __restrict__ A, const T* __restrict__ W, int ns, int m, int d, int64_t ld, int64_t ss,
                        const T* __restrict__ gamma, int q, T* __restrict__ mg, T* __restrict__ vg, int accumulate)
{
    int64_t idx;
    int lane;
    if (!wave_row((int64_t)ns * d, idx, lane)) return;
    const int64_t row = idx / d;
    const int e = (int)(idx - row * d);
    const T* w0 = W + row * ld;
    const T* we = w0 + (int64_t)(e + 1) * ss;
    const T* a0 = vg ? A + row * ld : nullptr;
    const T* ae = vg ? a0 + (int64_t)(e + 1) * ss : nullptr;
    double sv = 0.0, acc[MAXQ] = {};
    for (int j = lane; j < m; j += 64) {
        const double dw = (double)we[j];
        if (vg) sv += (double)w0[j] * dw - (double)a0[j] * (double)ae[j];
        if (mg) dot_step(acc, dw, gamma + (int64_t)j * q, q);
    }
    wave_sum(sv, acc);
    if (lane != 0) return;
    if (vg) put(vg + idx, (T)(2.0 * sv), accumulate);
    if (mg) {
#pragma unroll
        for (int c = 0; c < MAXQ; ++c)
            if (c < q) put(mg + idx * q + c, (T)acc[c], accumulate);
    }
}

// A wave per row, 4 rows per workgroup (wave_row); the lanes' partial sums are added by wave_sum.  lm or lv may be nullptr.
template <typename T>
__global__ __launch_bounds__(256)
void k_sparse_loo(const T* __restrict__ A, const T* __restrict__ V, int n, int m, int64_t ld, const T* __restrict__ gamma,
                  const T* __restrict__ r, int q, double sf2, double noise, int mode, T* __restrict__ lm, T* __restrict__ lv,
                  int32_t* __restrict__ bad)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    const T* a = A + (int64_t)row * ld;
    const T* v = V + (int64_t)row * ld;
    double sa = 0.0, sv = 0.0, acc[MAXQ] = {};
    for (int j = lane; j < m; j += 64) {
        const double av = (double)a[j], vv = (double)v[j];
        sa += av * av;
        sv += vv * vv;
        dot_step(acc, vv, gamma + (int64_t)j * q, q);
    }
    wave_sum(sa, sv, acc);
    if (lane != 0) return;
    const double lam = mode == 0 ? sf2 - sa + noise : noise;
    const double one_h = 1.0 - sv / lam;
    if (!(one_h > 0.0)) atomicAdd(bad, 1);
    if (lv) lv[row] = (T)(lam / one_h);
    if (lm) {
#pragma unroll
        for (int c = 0; c < MAXQ; ++c)
            if (c < q) {
                const double rc = (double)r[(int64_t)row * q + c];
                lm[(int64_t)row * q + c] = (T)(rc - (rc - acc[c]) / one_h);
            }
    }
}

// lower(C) += A A^T: one gemm_tile per workgroup over the tiles of the lower triangle (k_gemm_nt_sub's LOWER form with
// the positive sign of gemm_tile's ADD).
template <typename T, int W>
__global__ __launch_bounds__(256, 2)
void k_syrk_add_lower(T* __restrict__ C, int64_t ldc, const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb, int N,
                      int K)
{
    constexpr int GT = 32 * W;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * GT * LROW];
    int ti, tj;
    lower_tile_of((int)blockIdx.x, ti, tj);
    const bool interior = (ti + 1) * GT <= N && (K % (KT_BYTES / (int)sizeof(T))) == 0;
    if (interior) gemm_tile<T, true, false, W, true>(smem, C, ldc, A, lda, B, ldb, N, N, K, ti, tj);
    else          gemm_tile<T, true, true,  W, true>(smem, C, ldc, A, lda, B, ldb, N, N, K, ti, tj);
}

// the ns x ns block's strict upper triangle set to zero (after the factorisation)
template <typename T>
__global__ __launch_bounds__(256)
void k_zero_strict_upper(T* __restrict__ c, int64_t ldc, int64_t ns)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ns * ns) return;
    const int64_t i = e / ns, j = e - i * ns;
    if (j > i) c[i * ldc + j] = (T)0;
}

template <typename T, int W>
static int syrk_add_launch(T* c, int64_t ldc, const T* a, int64_t lda, int64_t n, int k, hipStream_t st, const char* fn)
{
    constexpr int GT = 32 * W;
    const int64_t tm = (n + GT - 1) / GT;
    hipLaunchKernelGGL((k_syrk_add_lower<T, W>), dim3((unsigned)(tm * (tm + 1) / 2)), dim3(256), 0, st, c, ldc, a, lda, a, lda, (int)n, k);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

// The tile edge by gemm_nt_sub's rule for a lower update of one problem, up to 64-tiles: the 128-tile instance of the
// lower form needs 10 registers more than the 256 a wave has at two workgroups per compute unit (hipcc spills them to
// scratch, as it does for the subtracting instance) and is not built here.
template <typename T>
static int syrk_add_lower(T* c, int64_t ldc, const T* a, int64_t lda, int64_t n, int k, hipStream_t st, const char* fn)
{
    const int64_t t64 = ((n + 63) / 64) * ((n + 63) / 64) / 2;
    if (n <= 32 || t64 < 32) return syrk_add_launch<T, 1>(c, ldc, a, lda, n, k, st, fn);
    return syrk_add_launch<T, 2>(c, ldc, a, lda, n, k, st, fn);
}

template <typename T, int COV>
static int cross_grad_run_cov(const T* xa, int64_t na, const T* xb, int64_t nb, int d, double ell, double sf2, T* out, int64_t ldo,
                              int64_t ss, hipStream_t st, const char* fn)
{
    const int64_t tm = (na + CG_TILE - 1) / CG_TILE, tn = (nb + CG_TILE - 1) / CG_TILE;
    const T c = (T)cov_scale(COV, ell);
    with_dim(d, [&](auto dd) {
        hipLaunchKernelGGL((k_cov_cross_grad<T, COV, decltype(dd)::value>), dim3((unsigned)(tm * tn)), dim3(256), 0, st, xa, (int)na, xb,
                           (int)nb, d, c, (T)sf2, out, ldo, ss, (int)tn);
    });
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
static int joint_cov_run(int cov, const T* xs, int64_t ns, int d, double ell, double sf2, double diag, const T* astar, const T* wstar,
                         int64_t m, int64_t ld, T* c, int64_t ldc, T* cws, int32_t* info, hipStream_t st, const char* fn)
{
    int rc = rbf_gram_run<T>(xs, ns, xs, ns, d, ell, sf2, diag, c, ldc, true, true, st, cov, fn);
    if (rc) return rc;
    rc = gemm_nt_sub<T>(c, ldc, astar, ld, astar, ld, ns, ns, (int)m, true, st);
    if (rc) return rc;
    rc = syrk_add_lower<T>(c, ldc, wstar, ld, ns, (int)m, st, fn);
    if (rc) return rc;
    if (cws == nullptr) return 0;
    rc = potrf_batched_run<T>(c, ns, ldc, cws, info, (T*)nullptr, 0, 0, PotrfBatch(), st);
    if (rc) return rc;
    hipLaunchKernelGGL((k_zero_strict_upper<T>), dim3((unsigned)((ns * ns + 255) / 256)), dim3(256), 0, st, c, ldc, ns);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_cov_cross_grad(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, double ell,
                          double sf2, void* out_dev, int64_t ldo, int64_t slab_stride, void* stream)
{
    const char* fn = "cimrgp_cov_cross_grad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(xa_dev && xb_dev && out_dev, fn, "null pointer");
    CIMRGP_REQUIRE(na >= 0 && na < (1ll << 30) && nb >= 0 && nb < (1ll << 30), fn, "na and nb must be in [0, 2^30)");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    CIMRGP_REQUIRE(ldo >= nb, fn, "leading dimension too small");
    CIMRGP_REQUIRE(na == 0 || slab_stride >= (na - 1) * ldo + nb, fn, "slab stride too small");
    CIMRGP_REQUIRE(((na + CG_TILE - 1) / CG_TILE) * ((nb + CG_TILE - 1) / CG_TILE) < (1ll << 31), fn, "grid too large");
    if (na == 0 || nb == 0) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return with_cov(cov, [&](auto cv) {
            return cross_grad_run_cov<T, decltype(cv)::value>((const T*)xa_dev, na, (const T*)xb_dev, nb, d, ell, sf2, (T*)out_dev, ldo,
                                                              slab_stride, stream_of(stream), fn);
        });
    });
}

int cimrgp_sparse_tail_grad(int dtype, const void* a_dev, const void* w_dev, int64_t ns, int64_t m, int d, int64_t ld,
                            int64_t slab_stride, const void* gamma_dev, int q, void* mean_grad_dev, void* var_grad_dev,
                            int accumulate, void* stream)
{
    const char* fn = "cimrgp_sparse_tail_grad";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(w_dev, fn, "null pointer");
    CIMRGP_REQUIRE(var_grad_dev == nullptr || a_dev, fn, "null pointer (a)");
    CIMRGP_REQUIRE(mean_grad_dev == nullptr || gamma_dev, fn, "null pointer (gamma)");
    CIMRGP_REQUIRE(ns >= 0 && ns < (1ll << 30) && m >= 1 && m < (1ll << 31) && ld >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(mean_grad_dev == nullptr || (q >= 1 && q <= MAXQ), fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(ns == 0 || slab_stride >= (ns - 1) * ld + m, fn, "slab stride too small");
    if (ns == 0 || (mean_grad_dev == nullptr && var_grad_dev == nullptr)) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_tail_grad<T>), dim3((unsigned)((ns * d + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)a_dev,
                           (const T*)w_dev, (int)ns, (int)m, d, ld, slab_stride, (const T*)gamma_dev, q, (T*)mean_grad_dev,
                           (T*)var_grad_dev, accumulate);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

int cimrgp_sparse_loo(int dtype, const void* a_dev, const void* v_dev, int64_t n, int64_t m, int64_t ld, const void* gamma_dev,
                      const void* r_dev, int q, double sf2, double noise, int mode, void* loo_mean_dev, void* loo_var_dev,
                      int32_t* bad_dev, void* stream)
{
    const char* fn = "cimrgp_sparse_loo";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(a_dev && v_dev && gamma_dev && r_dev && bad_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && n < (1ll << 31) && m >= 1 && m < (1ll << 31) && ld >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(mode == 0 || mode == 1, fn, "mode must be 0 (FITC) or 1 (VFE)");
    CIMRGP_REQUIRE(sf2 > 0.0 && noise > 0.0, fn, "sf2 and noise must be positive");
    if (n == 0) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_sparse_loo<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)a_dev,
                           (const T*)v_dev, (int)n, (int)m, ld, (const T*)gamma_dev, (const T*)r_dev, q, sf2, noise, mode,
                           (T*)loo_mean_dev, (T*)loo_var_dev, bad_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

int cimrgp_sparse_joint_cov(int dtype, int cov, const void* xs_dev, int64_t ns, int d, double ell, double sf2, double diag,
                            const void* astar_dev, const void* wstar_dev, int64_t m, int64_t ld, void* c_dev, int64_t ldc,
                            void* cws_dev, size_t cws_bytes, int32_t* info_dev, void* stream)
{
    const char* fn = "cimrgp_sparse_joint_cov";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(xs_dev && astar_dev && wstar_dev && c_dev, fn, "null pointer");
    CIMRGP_REQUIRE(cws_dev == nullptr || info_dev != nullptr, fn, "null pointer (info)");
    CIMRGP_REQUIRE(ns >= 0 && ns < (1ll << 30) && m >= 1 && m < (1ll << 31), fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    CIMRGP_REQUIRE(ld >= m && ldc >= ns && ldc >= 1, fn, "leading dimension too small");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ld % e == 0 && ldc % e == 0, fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(ld * (int64_t)elem_bytes(dtype) >= 128, fn, "leading dimension of A* and W* must span at least 128 bytes");
    CIMRGP_REQUIRE(aligned16(astar_dev) && aligned16(wstar_dev) && aligned16(c_dev) && aligned16(cws_dev), fn,
                   "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(cws_dev == nullptr || cws_bytes >= cimrgp_potrf_workspace_bytes(dtype, ns), fn, "factor workspace too small");
    if (ns == 0) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return joint_cov_run<T>(cov, (const T*)xs_dev, ns, d, ell, sf2, diag, (const T*)astar_dev, (const T*)wstar_dev, m, ld, (T*)c_dev,
                                ldc, (T*)cws_dev, info_dev, stream_of(stream), fn);
    });
}

}  // extern "C"
