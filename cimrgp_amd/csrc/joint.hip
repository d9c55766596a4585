// The joint predictive distribution of a layer's blocks (include/cimrgp_joint.h):
//   normal_fill   counter-based standard normals (Philox4x32-10 + Box-Muller), one value per (seed, key, column, point)
//   joint_cov     K(xs, xs) + diag - W W^T, W = K(xs, x) L^-T: the batched Gram, the shared cross-Gram and row solve
//                 (cross_solve_run, layer.hip), the batched lower update (gemm_nt_sub as a SYRK), optionally the
//                 batched factorisation and a zeroed strict upper triangle
//   layer_sample  out^T += Z^T L^T per block: k_layer_sample, gemm_tile's body with a positive sign, B read as lower
//                 triangular and K cut at the last row of each column tile (tiles above the diagonal are never
//                 computed: ns^2 cols flops instead of 2 ns^2 cols)
#include "abi.hpp"
#include "gemm_tile.hpp"

namespace cimrgp {

namespace {

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) ----
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

static __device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
        const uint32_t lo0 = PHILOX_M0 * ctr.x, hi0 = __umulhi(PHILOX_M0, ctr.x);
        const uint32_t lo1 = PHILOX_M1 * ctr.z, hi1 = __umulhi(PHILOX_M1, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0);
    }
    return ctr;
}

// one thread = one pair of points (2m, 2m + 1) of one column of one block: they share the Philox output
template <typename T>
__global__ __launch_bounds__(256)
void k_normal_fill(uint32_t seed_lo, uint32_t seed_hi, const uint64_t* __restrict__ keys, int64_t rows, int64_t cols, int64_t col0,
                   int64_t ns, T* __restrict__ z, int64_t ldz, int64_t zs)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = 2 * m;
    if (i >= ns) return;
    for (int64_t rc = blockIdx.y; rc < rows; rc += gridDim.y) {
        const int64_t b = rc / cols, c = rc - b * cols;
        const uint64_t key = keys[b];
        const uint4 x = philox4x32_10(make_uint4((uint32_t)m, (uint32_t)(col0 + c), (uint32_t)key, (uint32_t)(key >> 32)),
                                      seed_lo, seed_hi);
        const double u1 = ((double)(((uint64_t)x.y << 32 | x.x) >> 11) + 0.5) * 0x1p-53;
        const double u2 = ((double)(((uint64_t)x.w << 32 | x.z) >> 11) + 0.5) * 0x1p-53;
        const double r = sqrt(-2.0 * log(u1));
        const double a = 2.0 * M_PI * u2;
        T* dst = z + b * zs + c * ldz + i;
        dst[0] = (T)(r * cos(a));
        if (i + 1 < ns) dst[1] = (T)(r * sin(a));
    }
}

// lower(C_b) -> strict upper triangle of the ns x ns block set to zero (after the factorisation)
template <typename T>
__global__ void k_joint_zero_upper(T* __restrict__ c, int64_t ldc, int64_t cs, int64_t ns)
{
    const int64_t b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ns * ns) return;
    const int64_t i = e / ns, j = e - i * ns;
    if (j > i) c[b * cs + i * ldc + j] = (T)0;
}

// out[c][t_b + i] += sum_{k <= i} L_b[i][k] Z_b[c][k]: the NT product C (cols x ns) += A (= Z_b^T rows) B^T (B = L_b),
// one gemm_tile per workgroup, blockIdx.y = block.  Column tile tj needs K only up to its last row (L is lower
// triangular); tiles are dealt longest K first.  The triangle inside the last K stages is masked on the way into LDS
// (TRI_B), so the strict upper triangle of L is never used.  FP64 128-tiles: one workgroup per compute unit (with two,
// the triangle mask leaves hipcc 3 registers short of the 256 and it spills to scratch; with one, the accumulators
// move to the AGPRs and nothing spills).
template <typename T, int W>
__global__ __launch_bounds__(256, (W == 4 && sizeof(T) == 8) ? 1 : 2)
void k_layer_sample(const T* __restrict__ L, int64_t ldl, int64_t sl, int ns, const T* __restrict__ Z, int64_t ldz, int64_t sz,
                    int cols, const int64_t* __restrict__ t_starts, T* __restrict__ out, int64_t ld_out, int tiles_m, int tiles_n)
{
    constexpr int GT = 32 * W;
    constexpr int BKE = KT_BYTES / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * GT * LROW];
    const int64_t b = blockIdx.y;
    const int id = blockIdx.x;
    const int tjr = id / tiles_m;
    const int ti = id - tjr * tiles_m;
    const int tj = tiles_n - 1 - tjr;
    const int K = min(ns, (tj + 1) * GT);
    T* C = out + t_starts[b];
    const T* A = Z + b * sz;
    const T* B = L + b * sl;
    const bool interior = (ti + 1) * GT <= cols && (tj + 1) * GT <= ns && (K % BKE) == 0;
    if (interior) gemm_tile<T, false, false, W, true, true>(smem, C, ld_out, A, ldz, B, ldl, cols, ns, K, ti, tj);
    else          gemm_tile<T, false, true,  W, true, true>(smem, C, ld_out, A, ldz, B, ldl, cols, ns, K, ti, tj);
}

template <typename T, int W>
static int sample_launch(const T* l, int64_t ldl, int64_t sl, int64_t ns, int batch, const T* z, int64_t ldz, int64_t sz,
                         int64_t cols, const int64_t* t_starts, T* out, int64_t ld_out, hipStream_t st)
{
    constexpr int GT = 32 * W;
    const int64_t tm = (cols + GT - 1) / GT, tn = (ns + GT - 1) / GT;
    CIMRGP_REQUIRE(tm * tn < (1ll << 31), "cimrgp_layer_sample", "grid too large");
    hipLaunchKernelGGL((k_layer_sample<T, W>), dim3((unsigned)(tm * tn), (unsigned)batch), dim3(256), 0, st, l, ldl, sl, (int)ns, z,
                       ldz, sz, (int)cols, t_starts, out, ld_out, (int)tm, (int)tn);
    CIMRGP_LAUNCH_CHECK("cimrgp_layer_sample");
    return 0;
}

}  // namespace

template <typename T>
static int normal_fill_run(uint64_t seed, const uint64_t* keys, int batch, int64_t col0, int64_t cols, int64_t ns, T* z, int64_t ldz,
                           int64_t zs, hipStream_t st)
{
    if (cols == 0 || ns == 0) return 0;
    const int64_t rows = (int64_t)batch * cols;
    const unsigned gx = (unsigned)((ns + 511) / 512);
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    hipLaunchKernelGGL((k_normal_fill<T>), dim3(gx, gy), dim3(256), 0, st, (uint32_t)seed, (uint32_t)(seed >> 32), keys, rows, cols,
                       col0, ns, z, ldz, zs);
    CIMRGP_LAUNCH_CHECK("cimrgp_normal_fill");
    return 0;
}

template <typename T>
static int joint_cov_run(const LayerJoint<T>& a, hipStream_t st)
{
    const char* fn = "cimrgp_layer_joint_cov";
    const int64_t ns = a.te.n;
    const Arena<T>& c = a.c.l;
    if (ns <= 0) return 0;
    // lower(C_b) = K(xs_b, xs_b) + diag_b I
    int rc = rbf_gram_batched_run<T>(a.bc, a.te, a.te, a.diag, c, true, st);
    if (rc) return rc;
    // W_b = K(xs_b, x_b) L_b^-T
    rc = cross_solve_run<T>(a.bc, a.tr, a.f, a.te, a.w, st);
    if (rc) return rc;
    // lower(C_b) -= W_b W_b^T
    rc = gemm_nt_sub<T>(c.p, c.ld, a.w.p, a.w.ld, a.w.p, a.w.ld, ns, ns, (int)a.tr.n, true, st,
                        gemm_batch(a.bc.batch, c.stride, a.w.stride, a.w.stride));
    if (rc) return rc;
    if (a.c.ws == nullptr) return 0;
    rc = potrf_batched_run<T>(c.p, ns, c.ld, a.c.ws, a.info, (T*)nullptr, 0, 0, potrf_batch(a.bc.batch, a.c, 0), st);
    if (rc) return rc;
    hipLaunchKernelGGL((k_joint_zero_upper<T>), dim3((unsigned)((ns * ns + 255) / 256), (unsigned)a.bc.batch), dim3(256), 0, st, c.p,
                       c.ld, c.stride, ns);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
static int layer_sample_run(const T* l, int64_t ldl, int64_t sl, int64_t ns, int batch, const T* z, int64_t ldz, int64_t sz,
                            int64_t cols, const int64_t* t_starts, T* out, int64_t ld_out, hipStream_t st)
{
    if (ns <= 0 || cols <= 0) return 0;
    // tile edge by the number of workgroups a launch gets (gemm_nt_sub's rule): 128-tiles from ~3 per compute unit
    const int64_t t128 = ((cols + 127) / 128) * ((ns + 127) / 128) * batch;
    const int64_t t64 = ((cols + 63) / 64) * ((ns + 63) / 64) * batch;
    if (cols <= 32 || t64 < 32) return sample_launch<T, 1>(l, ldl, sl, ns, batch, z, ldz, sz, cols, t_starts, out, ld_out, st);
    if (t128 < 768 || cols <= 64) return sample_launch<T, 2>(l, ldl, sl, ns, batch, z, ldz, sz, cols, t_starts, out, ld_out, st);
    return sample_launch<T, 4>(l, ldl, sl, ns, batch, z, ldz, sz, cols, t_starts, out, ld_out, st);
}

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_normal_fill(int dtype, uint64_t seed, const uint64_t* keys_dev, int batch, int64_t col0, int64_t cols, int64_t ns,
                       void* z_dev, int64_t ldz, int64_t z_stride, void* stream)
{
    const char* fn = "cimrgp_normal_fill";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(keys_dev && z_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(cols >= 0 && ns >= 0 && col0 >= 0, fn, "negative size");
    CIMRGP_REQUIRE(col0 + cols <= (1ll << 32), fn, "column index beyond 2^32");
    CIMRGP_REQUIRE(ns < (1ll << 33), fn, "too many points");
    CIMRGP_REQUIRE(ldz >= ns && ldz >= 1, fn, "leading dimension of z smaller than ns");
    CIMRGP_REQUIRE(batch == 1 || cols == 0 || z_stride >= (cols - 1) * ldz + ns, fn, "block stride too small");
    CIMRGP_REQUIRE(cols * (int64_t)batch < (1ll << 40), fn, "too many columns");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return normal_fill_run<T>(seed, keys_dev, batch, col0, cols, ns, (T*)z_dev, ldz, z_stride, stream_of(stream));
    });
}

int cimrgp_layer_joint_cov(int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d, const void* xs_dev,
                           const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2, const void* l_arena_dev,
                           int64_t ldl, int64_t l_stride, const void* ws_arena_dev, size_t ws_stride_bytes, const void* diag_dev,
                           void* w_arena_dev, int64_t ldw, int64_t w_stride, void* c_arena_dev, int64_t ldc, int64_t c_stride,
                           void* cws_arena_dev, size_t cws_stride_bytes, int32_t* info_dev, void* stream)
{
    const char* fn = "cimrgp_layer_joint_cov";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(x_dev && starts_dev && xs_dev && t_starts_dev && l_arena_dev && ws_arena_dev && w_arena_dev && c_arena_dev, fn,
                   "null pointer");
    CIMRGP_REQUIRE(cws_arena_dev == nullptr || info_dev != nullptr, fn, "null pointer (info)");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 30) && ns >= 0 && ns < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    CIMRGP_REQUIRE(ldl >= n && ldw >= n && ldc >= ns && ldc >= 1, fn, "leading dimension too small");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldw % e == 0 && ldc % e == 0 && l_stride % e == 0 && w_stride % e == 0 && c_stride % e == 0, fn,
                   "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(ldw * (int64_t)elem_bytes(dtype) >= 128, fn, "leading dimension of W must span at least 128 bytes");
    CIMRGP_REQUIRE(batch == 1 || (block_stride_ok(l_stride, n, n, ldl) && block_stride_ok(w_stride, ns, n, ldw) &&
                                  block_stride_ok(c_stride, ns, ns, ldc)), fn, "block stride too small");
    CIMRGP_REQUIRE(aligned16(l_arena_dev) && aligned16(ws_arena_dev) && aligned16(w_arena_dev) && aligned16(c_arena_dev) &&
                   aligned16(cws_arena_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(ws_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace stride too small");
    CIMRGP_REQUIRE(cws_arena_dev == nullptr ||
                   workspace_stride_ok(dtype, ns, cws_stride_bytes), fn,
                   "factor workspace stride too small or misaligned");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerJoint<T> a;
        a.bc = BatchCov{batch, d, cov, ell, sf2};
        a.tr = Points<T>{(const T*)x_dev, starts_dev, n};
        a.te = Points<T>{(const T*)xs_dev, t_starts_dev, ns};
        a.f = Factors<const T>{{(const T*)l_arena_dev, ldl, l_stride}, (const T*)ws_arena_dev, (int64_t)(ws_stride_bytes / sizeof(T))};
        a.diag = (const T*)diag_dev;
        a.w = Arena<T>{(T*)w_arena_dev, ldw, w_stride};
        a.c = Factors<T>{{(T*)c_arena_dev, ldc, c_stride}, (T*)cws_arena_dev, (int64_t)(cws_stride_bytes / sizeof(T))};
        a.info = info_dev;
        return joint_cov_run<T>(a, stream_of(stream));
    });
}

int cimrgp_layer_sample(int dtype, const void* l_arena_dev, int64_t ldl, int64_t l_stride, int64_t ns, int batch, const void* z_dev,
                        int64_t ldz, int64_t z_stride, int64_t cols, const int64_t* t_starts_dev, void* out_dev, int64_t ld_out,
                        void* stream)
{
    const char* fn = "cimrgp_layer_sample";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(l_arena_dev && z_dev && t_starts_dev && out_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536, fn, "batch count out of range");
    CIMRGP_REQUIRE(cols >= 0 && ns >= 0 && cols < (1ll << 30) && ns < (1ll << 30), fn, "bad dimensions");
    CIMRGP_REQUIRE(ldl >= ns && ldz >= ns && ld_out >= 1 && ldl < (1ll << 23) && ldz < (1ll << 23), fn, "bad leading dimension");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldz % e == 0 && l_stride % e == 0 && z_stride % e == 0, fn,
                   "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(ldl * (int64_t)elem_bytes(dtype) >= 128 && ldz * (int64_t)elem_bytes(dtype) >= 128, fn,
                   "leading dimensions must span at least 128 bytes (a K stage of the tile loads 128 bytes per row)");
    CIMRGP_REQUIRE(aligned16(l_arena_dev) && aligned16(z_dev), fn, "pointers must be 16-byte aligned");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return layer_sample_run<T>((const T*)l_arena_dev, ldl, l_stride, ns, batch, (const T*)z_dev, ldz, z_stride, cols, t_starts_dev,
                                   (T*)out_dev, ld_out, stream_of(stream));
    });
}

}  // extern "C"
