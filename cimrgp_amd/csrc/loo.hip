// Leave-one-out cross-validation of a fitted block and the triangular inverse behind it (include/cimrgp_loo.h):
//   trtri_rows   rows [r0, r0 + m) of U = L^-T: the forward row solve B <- B L^-T on rows of the identity, panels of 256
//                columns from panel r0 / 256 on, rows joining at their own panel (nothing left of a row's diagonal is
//                computed):
//                  k_loo_init     the strip's columns [r0, n) <- rows of the identity
//                  k_loo_diag     U[rows <= p, p] <- U[rows <= p, p] L_pp^-T   (32-row strips of the panel in LDS, in
//                                 place; L_pp^-T is the block the factorisation left in its workspace, read as upper
//                                 triangular: k runs to the column tile's last column only)
//                  k_loo_update   U[rows <= p, > p] -= U[rows <= p, p] L[> p, p]^T   (gemm_tile's body, K = 256)
//                both on the matrix cores (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Mx<T> in common.hpp)
//   kinv_diag    strips of trtri_rows through a scratch buffer, each reduced by k_loo_rowsq (a workgroup per row, from
//                the row's own panel on, fixed order)
//   loo          k_loo_tail: y - alpha / d, 1 / d
// A row's values depend on its global index alone (tiles and strips are aligned to global row numbers, every K loop
// has a fixed order): the result is bit-identical whatever the strip height.
#include "abi.hpp"
#include "reduce.hpp"
#include "gemm_tile.hpp"

namespace cimrgp {

namespace {

constexpr int LD_ROWS = 32;      // rows per workgroup of k_loo_diag

// ------------------------------------------------------------------- rows of the identity ----
// blockIdx.x = row of the strip, blockIdx.y = block.  Columns [r0, n).
template <typename T>
__global__ __launch_bounds__(256)
void k_loo_init(T* __restrict__ U, int64_t ldu, int64_t su, int r0, int n)
{
    U += (int64_t)blockIdx.y * su + (int64_t)blockIdx.x * ldu;
    const int diag = r0 + (int)blockIdx.x;
    for (int c = r0 + (int)threadIdx.x; c < n; c += 256) U[c] = (c == diag) ? (T)1 : (T)0;
}

// -------------------------------------------------------- U[:, p] <- U[:, p] L_pp^-T ----
// One workgroup = 32 rows of the strip and the whole panel (w <= 256 columns): the rows are read into LDS before
// anything is written, so the product goes back in place.  Wave v owns output columns [64 v, 64 v + 64): two row tiles
// by four column tiles.  (L_pp^-T)[k][j] = invT[k][j], zero for k > j: the right operand's fragment (B^T[col][kslot])
// is invT[kslot][col] -- for one k the 16 lanes of a column tile read one contiguous segment; the 256 x 256 block is
// shared by every workgroup and stays in the caches -- masked to k <= col (the block's lower triangle is not trusted),
// and the K loop of a wave ends at its last column.
template <typename T>
__global__ __launch_bounds__(256)
void k_loo_diag(T* __restrict__ U, int64_t ldu, int64_t su, int mrows, int c0, int w, const T* __restrict__ invT, int64_t sws)
{
    using X = Mx<T>;
    using acc_t = typename X::acc_t;
    constexpr int LDS_LD = CIMRGP_NB + 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T strip[LD_ROWS * LDS_LD];
    U += (int64_t)blockIdx.y * su;
    invT += (int64_t)blockIdx.y * sws;
    const int row0 = (int)blockIdx.x * LD_ROWS;
    const int rows = min(LD_ROWS, mrows - row0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < LD_ROWS * CIMRGP_NB; e += 256) {
        const int r = e >> 8, c = e & (CIMRGP_NB - 1);
        strip[r * LDS_LD + c] = (r < rows && c < w) ? U[(int64_t)(row0 + r) * ldu + c0 + c] : (T)0;
    }
    __syncthreads();
    const int j0 = wave * 64;
    if (j0 >= w) return;
    acc_t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = acc_zero<T>();
    const int frow = lane & 15, fslot = lane >> 4;
    constexpr int KSTEP = 4 * X::EPS;
    const int kend = min(w, j0 + 64);
    // The right operand comes straight from global memory (L2).  K is walked in chunks of DK_STEPS k steps: all the
    // chunk's loads are issued first (unconditional, from clamped addresses inside the panel's w x w block), then its
    // multiplies -- one step at a time, every multiply waits a full memory round trip (64 steps per launch in FP64).
    // Steps past kend multiply by zeros (k > col is masked): they add exactly 0.
    constexpr int DK_STEPS = 8;
    int colc[4];
    bool colok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        colc[t] = min(j0 + 16 * t + frow, w - 1);
        colok[t] = j0 + 16 * t + frow < w;
    }
    for (int kc = 0; kc < kend; kc += DK_STEPS * KSTEP) {
        T bv[DK_STEPS][4][X::EPS];
#pragma unroll
        for (int s = 0; s < DK_STEPS; ++s) {
            const int kk = kc + s * KSTEP + fslot * X::EPS;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < X::EPS; ++e) bv[s][t][e] = invT[min(kk + e, w - 1) * CIMRGP_NB + colc[t]];
        }
#pragma unroll
        for (int s = 0; s < DK_STEPS; ++s) {
            const int kk = kc + s * KSTEP + fslot * X::EPS;
            uint2 a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const uint2*>(&strip[(16 * i + frow) * LDS_LD + kk]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                T v[2] = {(T)0, (T)0};
#pragma unroll
                for (int e = 0; e < X::EPS; ++e) v[e] = (colok[t] && kk + e <= j0 + 16 * t + frow) ? bv[s][t][e] : (T)0;
                uint2 b;
                if constexpr (sizeof(T) == 8) {
                    b = *reinterpret_cast<const uint2*>(&v[0]);
                } else {
                    b.x = __float_as_uint((float)v[0]);
                    b.y = __float_as_uint((float)v[1]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][t] = X::mma(a[i], b, acc[i][t]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = j0 + 16 * t + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + X::crow(lane, r);
                if (row < rows && col < w) U[(int64_t)(row0 + row) * ldu + c0 + col] = acc[i][t][r];
            }
        }
}

// ------------------------------------------------- U[:, > p] -= U[:, p] L[> p, p]^T ----
// C (M x N) -= A (M x 256) B (N x 256)^T: C = the strip's columns right of the panel, A = its panel columns, B = the
// rows of L below the panel, its panel columns (strictly below the diagonal block: L's upper triangle is never read).
// One gemm_tile per workgroup, blockIdx.y = block.  K (= 256) is a kernel argument, not a constant: with a constant the
// compiler unrolls the stage loop and the FP64 128-tile spills.
template <typename T, int W>
__global__ __launch_bounds__(256, 2)
void k_loo_update(T* __restrict__ U, int64_t ldu, int64_t su, int M, int N, int c0, const T* __restrict__ L, int64_t ldl, int64_t sl,
                  int tiles_m, int K)
{
    constexpr int GT = 32 * W;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * GT * LROW];
    U += (int64_t)blockIdx.y * su;
    L += (int64_t)blockIdx.y * sl;
    const int id = blockIdx.x;
    const int tj = id / tiles_m, ti = id - tj * tiles_m;
    T* C = U + c0 + CIMRGP_NB;
    const T* A = U + c0;
    const T* B = L + (int64_t)(c0 + CIMRGP_NB) * ldl + c0;
    const bool interior = (ti + 1) * GT <= M && (tj + 1) * GT <= N;
    if (interior) gemm_tile<T, false, false, W>(smem, C, ldu, A, ldu, B, ldl, M, N, K, ti, tj);
    else          gemm_tile<T, false, true,  W>(smem, C, ldu, A, ldu, B, ldl, M, N, K, ti, tj);
}

// ---------------------------------------------------------------- row sums of squares ----
// One workgroup per row of the strip (blockIdx.y = block): thread t sums the squares of columns first + t, first + t +
// 256, ... (first = the row's own panel: what lies left of it is structurally zero and is not read), then the 256
// partial sums are added pairwise in LDS (lds_tree, reduce.hpp).  The order depends on the row's global index alone.
template <typename T>
__global__ __launch_bounds__(256)
void k_loo_rowsq(const T* __restrict__ U, int64_t ldu, int64_t su, int r0, int n, T* __restrict__ out, int64_t so)
{
    __shared__ double red[256];
    const int g = r0 + (int)blockIdx.x;
    const T* row = U + (int64_t)blockIdx.y * su + (int64_t)blockIdx.x * ldu;
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int c = (g & ~(CIMRGP_NB - 1)) + tid; c < n; c += 256) {
        const double v = (double)row[c];
        s += v * v;
    }
    red[tid] = s;
    lds_tree<256>(red, tid);
    if (tid == 0) out[(int64_t)blockIdx.y * so + g] = (T)red[0];
}

// ------------------------------------------------------------------------- the tail ----
template <typename T>
__global__ __launch_bounds__(256)
void k_loo_tail(const T* __restrict__ y, const int64_t* __restrict__ starts, const T* __restrict__ alpha, const T* __restrict__ diag,
                int n, int q, T* __restrict__ mean, T* __restrict__ var)
{
    const int64_t b = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const int64_t row = (starts ? starts[b] : 0) + i;
    const T d = diag[b * n + i];
    if (var) var[row] = (T)1 / d;
    if (mean) {
        for (int c = 0; c < q; ++c) mean[row * q + c] = y[row * q + c] - alpha[(b * n + i) * q + c] / d;
    }
}

// 128-tiles once a mid-sweep update has ~3 of them per compute unit (gemm_nt_sub's rule), 64-tiles below; a rule of n
// and the batch count alone, so that every strip of a matrix is cut the same way.
static inline bool loo_tile128(int64_t n, int batch) { return n * n * (int64_t)batch >= 768ll * 65536; }

}  // namespace

// rows [r0, r0 + m) of L^-T for bt.count blocks (strides bt.sk of L, bt.sws of the workspace, bt.sb of U, in elements)
template <typename T>
static int trtri_rows_run(const T* l, int64_t n, int64_t ldl, const T* ws, int64_t r0, int64_t m, T* u, int64_t ldu, hipStream_t st,
                          PotrfBatch bt, const char* fn)
{
    if (n <= 0 || m <= 0) return 0;
    const int64_t npan = (n + CIMRGP_NB - 1) / CIMRGP_NB;
    const T* invT = ws + ws_invT_offset(n);
    const unsigned nb = (unsigned)bt.count;
    const bool big = loo_tile128(n, bt.count);
    const int GT = big ? 128 : 64;
    CIMRGP_REQUIRE(m < (1ll << 31) && ((m + GT - 1) / GT) * (n / GT + 1) < (1ll << 31), fn, "grid too large");
    hipLaunchKernelGGL((k_loo_init<T>), dim3((unsigned)m, nb), dim3(256), 0, st, u, ldu, bt.sb, (int)r0, (int)n);
    CIMRGP_LAUNCH_CHECK(fn);
    for (int64_t p = r0 / CIMRGP_NB; p < npan; ++p) {
        const int64_t c0 = p * CIMRGP_NB;
        const int w = (int)std::min<int64_t>(CIMRGP_NB, n - c0);
        const int64_t mrows = std::min<int64_t>(m, c0 + w - r0);       // the strip's rows of the panels <= p
        hipLaunchKernelGGL((k_loo_diag<T>), dim3((unsigned)((mrows + LD_ROWS - 1) / LD_ROWS), nb), dim3(256), 0, st, u, ldu, bt.sb,
                           (int)mrows, (int)c0, w, invT + p * (CIMRGP_NB * CIMRGP_NB), bt.sws);
        CIMRGP_LAUNCH_CHECK(fn);
        const int64_t right = n - c0 - w;
        if (right <= 0) continue;
        const int64_t tiles_m = (mrows + GT - 1) / GT, tiles_n = (right + GT - 1) / GT;
        if (big)
            hipLaunchKernelGGL((k_loo_update<T, 4>), dim3((unsigned)(tiles_m * tiles_n), nb), dim3(256), 0, st, u, ldu, bt.sb, (int)mrows,
                               (int)right, (int)c0, l, ldl, bt.sk, (int)tiles_m, CIMRGP_NB);
        else
            hipLaunchKernelGGL((k_loo_update<T, 2>), dim3((unsigned)(tiles_m * tiles_n), nb), dim3(256), 0, st, u, ldu, bt.sb, (int)mrows,
                               (int)right, (int)c0, l, ldl, bt.sk, (int)tiles_m, CIMRGP_NB);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    return 0;
}

static inline int64_t loo_ldu(int64_t n) { return (n + 15) / 16 * 16; }
static inline int64_t loo_round256(int64_t v) { return (v + CIMRGP_NB - 1) / CIMRGP_NB * CIMRGP_NB; }

template <typename T>
static int kinv_diag_run(const T* l, int64_t n, int64_t ldl, const T* ws, T* scratch, int64_t strip, T* diag, hipStream_t st,
                         PotrfBatch bt, const char* fn)
{
    const int64_t ldu = loo_ldu(n);
    bt.sb = strip * ldu;
    for (int64_t r0 = 0; r0 < n; r0 += strip) {
        const int64_t m = std::min<int64_t>(strip, n - r0);
        int rc = trtri_rows_run<T>(l, n, ldl, ws, r0, m, scratch, ldu, st, bt, fn);
        if (rc) return rc;
        hipLaunchKernelGGL((k_loo_rowsq<T>), dim3((unsigned)m, (unsigned)bt.count), dim3(256), 0, st, (const T*)scratch, ldu, bt.sb,
                           (int)r0, (int)n, diag, n);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    return 0;
}

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_trtri_rows(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, int64_t r0, int64_t m,
                      void* u_dev, int64_t ldu, void* stream)
{
    const char* fn = "cimrgp_trtri_rows";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(l_dev && workspace_dev && u_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 30) && m >= 0, fn, "bad dimensions");
    CIMRGP_REQUIRE(r0 >= 0 && r0 % CIMRGP_NB == 0, fn, "r0 must be a multiple of 256");
    CIMRGP_REQUIRE(r0 <= n && m <= n - r0, fn, "rows [r0, r0 + m) must lie in [0, n)");
    CIMRGP_REQUIRE(ldl >= n && ldu >= n, fn, "leading dimension too small");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldu % e == 0, fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(l_dev) && aligned16(workspace_dev) && aligned16(u_dev), fn, "pointers must be 16-byte aligned");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return trtri_rows_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, r0, m, (T*)u_dev, ldu, stream_of(stream), PotrfBatch(),
                                 fn);
    });
}

size_t cimrgp_kinv_diag_scratch_bytes(int dtype, int64_t n, int64_t strip_rows)
{
    if (!dtype_known(dtype) || n < 1 || n >= (1ll << 30)) return 0;
    const int64_t top = loo_round256(n);
    int64_t strip = strip_rows < CIMRGP_NB ? CIMRGP_NB : (strip_rows > top ? top : loo_round256(strip_rows));
    return (size_t)(strip * loo_ldu(n)) * elem_bytes(dtype);
}

static int kinv_diag_entry(const char* fn, int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride,
                           const void* workspace_dev, size_t workspace_stride_bytes, void* scratch_dev, size_t scratch_bytes,
                           void* diag_out_dev, int batch, void* stream)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(l_dev && workspace_dev && scratch_dev && diag_out_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(ldl >= n, fn, "leading dimension too small");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && l_stride % e == 0, fn, "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(l_dev) && aligned16(workspace_dev) && aligned16(scratch_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n) || batch == 1, fn, "workspace stride too small");
    CIMRGP_REQUIRE(workspace_stride_bytes % 16 == 0 || batch == 1, fn, "workspace stride must be a multiple of 16 bytes");
    CIMRGP_REQUIRE(batch == 1 || block_stride_ok(l_stride, n, n, ldl), fn, "block stride too small");
    const size_t row_bytes = (size_t)loo_ldu(n) * elem_bytes(dtype);
    CIMRGP_REQUIRE(scratch_bytes / (size_t)batch >= (size_t)CIMRGP_NB * row_bytes, fn, "scratch too small");
    int64_t strip = (int64_t)(scratch_bytes / (size_t)batch / row_bytes) / CIMRGP_NB * CIMRGP_NB;
    strip = std::min<int64_t>(strip, loo_round256(n));
    const PotrfBatch bt{batch, l_stride, (int64_t)(workspace_stride_bytes / elem_bytes(dtype)), 0};
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return kinv_diag_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)scratch_dev, strip, (T*)diag_out_dev,
                                stream_of(stream), bt, fn);
    });
}

int cimrgp_kinv_diag_batched(int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride, const void* workspace_dev,
                             size_t workspace_stride_bytes, void* scratch_dev, size_t scratch_bytes, void* diag_out_dev, int batch,
                             void* stream)
{
    return kinv_diag_entry("cimrgp_kinv_diag_batched", dtype, l_dev, n, ldl, l_stride, workspace_dev, workspace_stride_bytes, scratch_dev,
                           scratch_bytes, diag_out_dev, batch, stream);
}

int cimrgp_kinv_diag(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* scratch_dev,
                     size_t scratch_bytes, void* diag_out_dev, void* stream)
{
    return kinv_diag_entry("cimrgp_kinv_diag", dtype, l_dev, n, ldl, 0, workspace_dev, 0, scratch_dev, scratch_bytes, diag_out_dev, 1,
                           stream);
}

static int loo_entry(const char* fn, int dtype, const void* y_dev, const int64_t* starts_dev, const void* alpha_dev, const void* diag_dev,
                     int64_t n, int q, int batch, void* mean_out_dev, void* var_out_dev, void* stream)
{
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(diag_dev, fn, "null pointer");
    CIMRGP_REQUIRE(mean_out_dev == nullptr || (y_dev && alpha_dev), fn, "null pointer (y or alpha)");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n >= 0 && n < (1ll << 31), fn, "bad dimensions");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    if (n == 0 || (mean_out_dev == nullptr && var_out_dev == nullptr)) return 0;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)batch);
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((k_loo_tail<T>), grid, dim3(256), 0, stream_of(stream), (const T*)y_dev, starts_dev, (const T*)alpha_dev,
                           (const T*)diag_dev, (int)n, q, (T*)mean_out_dev, (T*)var_out_dev);
        CIMRGP_LAUNCH_CHECK(fn);
        return 0;
    });
}

int cimrgp_loo_batched(int dtype, const void* y_dev, const int64_t* starts_dev, const void* alpha_dev, const void* diag_dev, int64_t n,
                       int q, int batch, void* mean_out_dev, void* var_out_dev, void* stream)
{
    CIMRGP_REQUIRE(starts_dev != nullptr, "cimrgp_loo_batched", "null pointer (starts)");
    return loo_entry("cimrgp_loo_batched", dtype, y_dev, starts_dev, alpha_dev, diag_dev, n, q, batch, mean_out_dev, var_out_dev, stream);
}

int cimrgp_loo(int dtype, const void* y_dev, const void* alpha_dev, const void* diag_dev, int64_t n, int q, void* mean_out_dev,
               void* var_out_dev, void* stream)
{
    return loo_entry("cimrgp_loo", dtype, y_dev, nullptr, alpha_dev, diag_dev, n, q, 1, mean_out_dev, var_out_dev, stream);
}

}  // extern "C"
