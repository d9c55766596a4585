// The variational sparse GP's row pass (include/cimrgp_svgp.h):
//   svgp_rows  k_svgp_rows (a wave per row: m_i, v_i, then the Gauss-Hermite sum of log p(y_i | f) and its derivatives,
//              one node per lane), then k_svgp_partial and k_svgp_final (the three sums over the rows in a fixed order)
//
// k_svgp_rows.  The row walk is k_sparse_tail's (wave_row, wave_sum; reduce.hpp): lane l adds columns l, l + 64, .. of
// the row of A and of W in FP64 and the butterfly leaves the three row sums in EVERY lane.  Lane h < H then evaluates node
// h -- all of it FP64, for both dtypes -- and the same butterfly adds the four node sums (lanes >= H add zeros).  The
// likelihood is a compile-time policy (Lik<ID>): its constant term is evaluated once on the host.  No LDS, no atomics.
#include <cmath>

#include "abi.hpp"
#include "reduce.hpp"

namespace cimrgp {

namespace {

// log p(y | f) = c0 + body(e), e = y - f: `df` = d log p / d f, `ds` = d log p / d log s2.
template <int ID> struct Lik;

template <> struct Lik<CIMRGP_LIK_GAUSSIAN> {
    static double constant(double s2, double) { return -0.5 * std::log(2.0 * M_PI * s2); }
    static __device__ __forceinline__ void eval(double e, double s2, double, double c0, double& lp, double& df, double& ds)
    {
        const double z = e / s2;
        lp = c0 - 0.5 * e * z;
        df = z;
        ds = 0.5 * e * z - 0.5;
    }
};

template <> struct Lik<CIMRGP_LIK_STUDENT_T> {
    static double constant(double s2, double nu)
    {
        return std::lgamma(0.5 * (nu + 1.0)) - std::lgamma(0.5 * nu) - 0.5 * std::log(nu * M_PI * s2);
    }
    static __device__ __forceinline__ void eval(double e, double s2, double nu, double c0, double& lp, double& df, double& ds)
    {
        const double e2 = e * e, ns = nu * s2;
        lp = c0 - 0.5 * (nu + 1.0) * log1p(e2 / ns);
        df = (nu + 1.0) * e / (ns + e2);
        ds = 0.5 * (nu + 1.0) * e2 / (ns + e2) - 0.5;
    }
};

// rows: 3 n doubles, [E_i | dE_i / dlog s2 | 1 for a counted row], or nullptr (the scratch's first part).
template <typename T, int LIK>
__global__ __launch_bounds__(256)
void k_svgp_rows(const T* __restrict__ A, const T* __restrict__ W, int n, int m, int64_t ld, const T* __restrict__ gamma,
                 const T* __restrict__ kdiag, const T* __restrict__ y, int64_t ys, const double* __restrict__ nodes, int H, double s2,
                 double nu, double c0, T* __restrict__ mean, T* __restrict__ var, T* __restrict__ g1, T* __restrict__ g2,
                 double* __restrict__ rows)
{
    int row, lane;
    if (!wave_row(n, row, lane)) return;
    const T* a = A + (int64_t)row * ld;
    const T* w = W + (int64_t)row * ld;
    double sa = 0.0, sw = 0.0, mu = 0.0;
    for (int j = lane; j < m; j += 64) {
        const double av = (double)a[j], wv = (double)w[j];
        sa += av * av;
        sw += wv * wv;
        mu += wv * (double)gamma[j];
    }
    wave_sum(sa, sw, mu);
    const double v = (double)kdiag[row] - sa + sw;
    const bool ok = v > 0.0;                             // false for a NaN too
    double se = 0.0, s1 = 0.0, s2x = 0.0, ss = 0.0;
    double root = 1.0;
    if (ok) root = sqrt(2.0 * v);
    if (ok && lane < H) {
        const double x = nodes[lane], om = nodes[H + lane];
        double lp, df, ds;
        Lik<LIK>::eval((double)y[(int64_t)row * ys] - (mu + root * x), s2, nu, c0, lp, df, ds);
        se = om * lp;
        s1 = om * df;
        s2x = om * df * x;
        ss = om * ds;
    }
    wave_sum(se, s1, s2x, ss);
    if (lane != 0) return;
    constexpr double RSQRT_PI = 0.56418958354775628695;
    if (mean) mean[row] = (T)mu;
    if (var) var[row] = (T)v;
    if (g1) g1[row] = (T)(RSQRT_PI * s1);
    if (g2) g2[row] = (T)(RSQRT_PI * s2x / root);
    if (rows) {
        rows[row] = RSQRT_PI * se;
        rows[(int64_t)n + row] = RSQRT_PI * ss;
        rows[2 * (int64_t)n + row] = ok ? 0.0 : 1.0;
    }
}

// The three sums over the rows in two stages, in an order that depends on n alone.  k_svgp_partial: workgroup b adds
// the SV_CHUNK rows from b SV_CHUNK on -- thread t takes rows t, t + 256, .. of them, the 256 partial sums are added pairwise
// in LDS (lds_tree, reduce.hpp), the three columns together -- and writes part[3 b + c].  k_svgp_final: one workgroup adds
// the workgroups' sums the same way.  (One workgroup over all n rows, as k_sparse_sums has it, reads at one compute unit's
// rate: measured 0.036 ms beside a row pass of 0.224 ms at n = 65536, m = 1000.)
constexpr int SV_CHUNK = CIMRGP_SVGP_SUM_CHUNK;

__global__ __launch_bounds__(256)
void k_svgp_partial(const double* __restrict__ rows, int n, double* __restrict__ part)
{
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * SV_CHUNK;
    const int64_t end = base + SV_CHUNK < n ? base + SV_CHUNK : n;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = base + tid; i < end; i += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += rows[(int64_t)c * n + i];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][tid] = s[c];
    lds_tree<256, 3>(&red[0][0], tid);
    if (tid < 3) part[3 * (int64_t)blockIdx.x + tid] = red[tid][0];
}

__global__ __launch_bounds__(256)
void k_svgp_final(const double* __restrict__ part, int nparts, double* __restrict__ sums)
{
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = tid; b < nparts; b += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += part[3 * (int64_t)b + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][tid] = s[c];
    lds_tree<256, 3>(&red[0][0], tid);
    if (tid < 3) sums[tid] = red[tid][0];
}

// f(integral_constant<int, ID>) for the likelihood id `lik`, which the caller has checked.
template <typename F> static inline int with_likelihood(int lik, F&& f)
{
    if (lik == CIMRGP_LIK_GAUSSIAN) return f(std::integral_constant<int, CIMRGP_LIK_GAUSSIAN>());
    return f(std::integral_constant<int, CIMRGP_LIK_STUDENT_T>());
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

int cimrgp_svgp_rows(int dtype, const void* a_dev, const void* w_dev, int64_t n, int64_t m, int64_t ld, const void* gamma_dev,
                     const void* kdiag_dev, const void* y_dev, int64_t y_stride, const double* nodes_dev, int nodes, int likelihood,
                     double s2, double nu, void* mean_dev, void* var_dev, void* g1_dev, void* g2_dev, double* sums_dev,
                     double* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_svgp_rows";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(a_dev && w_dev && gamma_dev && kdiag_dev && y_dev && nodes_dev, fn, "null pointer");
    CIMRGP_REQUIRE(sums_dev == nullptr || scratch_dev != nullptr, fn, "null pointer (scratch)");
    CIMRGP_REQUIRE(n >= 1 && n < (1ll << 31) && m >= 1 && m < (1ll << 31) && ld >= m, fn, "bad dimensions");
    CIMRGP_REQUIRE(y_stride >= 1, fn, "y_stride must be positive");
    CIMRGP_REQUIRE(nodes >= 1 && nodes <= CIMRGP_SVGP_MAX_NODES, fn, "number of nodes must be in [1, 64]");
    CIMRGP_REQUIRE(likelihood == CIMRGP_LIK_GAUSSIAN || likelihood == CIMRGP_LIK_STUDENT_T, fn, "unknown likelihood");
    CIMRGP_REQUIRE(s2 > 0.0, fn, "the likelihood's scale must be positive");
    CIMRGP_REQUIRE(likelihood != CIMRGP_LIK_STUDENT_T || nu > 0.0, fn, "the degrees of freedom must be positive");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return with_likelihood(likelihood, [&](auto id) {
            constexpr int LIK = decltype(id)::value;
            double* rows = sums_dev ? scratch_dev : nullptr;
            hipLaunchKernelGGL((k_svgp_rows<T, LIK>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream_of(stream), (const T*)a_dev,
                               (const T*)w_dev, (int)n, (int)m, ld, (const T*)gamma_dev, (const T*)kdiag_dev, (const T*)y_dev, y_stride,
                               nodes_dev, nodes, s2, nu, Lik<LIK>::constant(s2, nu), (T*)mean_dev, (T*)var_dev, (T*)g1_dev, (T*)g2_dev,
                               rows);
            CIMRGP_LAUNCH_CHECK(fn);
            if (sums_dev) {
                const int64_t nparts = (n + SV_CHUNK - 1) / SV_CHUNK;
                double* part = rows + 3 * n;
                hipLaunchKernelGGL(k_svgp_partial, dim3((unsigned)nparts), dim3(256), 0, stream_of(stream), (const double*)rows, (int)n, part);
                CIMRGP_LAUNCH_CHECK(fn);
                hipLaunchKernelGGL(k_svgp_final, dim3(1), dim3(256), 0, stream_of(stream), (const double*)part, (int)nparts, sums_dev);
                CIMRGP_LAUNCH_CHECK(fn);
            }
            return 0;
        });
    });
}

}  // extern "C"
