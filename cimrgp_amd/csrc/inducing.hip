// Greedy inducing-point selection: the matrix-free pivoted Cholesky factorisation of include/cimrgp_inducing.h
// ("Greedy inducing-point selection").  FP64 only.  Per step two plain launches in stream order:
//   k_pc_column  one workgroup (four waves) per PC_ROWS = 64 rows: the pivot row's earlier coefficients come through LDS in
//                chunks; wave w adds columns t = w, w + 4, .. of its 64 rows (a 512-byte run per load, eight loads in
//                flight per lane), the four partial sums meet in LDS in wave order (sum4), and wave 0 forms the new column,
//                the residuals and the workgroup's (arg-max, trace) record.
//   k_pc_pick    ONE workgroup: the records in a fixed order -> the next pivot, its residual, the trace entry, the rank
//                count, and the gather of the next pivot row's earlier coefficients into a contiguous vector.
// No workgroup waits on another, nothing is atomic, the pivot never leaves the device.
#include "abi.hpp"
#include "reduce.hpp"

#include <math.h>

namespace cimrgp {

namespace {

constexpr int PC_ROWS = CIMRGP_PIVCHOL_ROWS;    // rows per workgroup of k_pc_column and per record
constexpr int PC_CHUNK = 1024;                  // earlier coefficients of the pivot row staged in LDS at a time (a multiple of 4)
constexpr int PC_UNROLL = 8;                    // loads in flight per lane in the column pass
constexpr int PC_NONE = 0x7fffffff;             // the row index of "no candidate": it loses every tie

// the pivot of the current step: written by k_pc_pick, read by k_pc_column
struct PcState { int64_t p; double dp; };

struct PcScratch { size_t prow = 0, mark = 0, val = 0, tr = 0, idx = 0, state = 0, total = 0; };

static inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
static inline int64_t pc_records(int64_t n) { return (n + PC_ROWS - 1) / PC_ROWS; }
static inline bool pc_sizes_ok(int64_t n, int64_t m) { return m >= 1 && m <= n && n < ((int64_t)1 << 31); }

static PcScratch pc_scratch(int64_t n, int64_t m)
{
    PcScratch s;
    const size_t rec = (size_t)pc_records(n);
    s.prow = 0;
    s.mark = s.prow + up16((size_t)m * sizeof(double));
    s.val = s.mark + up16((size_t)n * sizeof(int32_t));
    s.tr = s.val + up16(rec * sizeof(double));
    s.idx = s.tr + up16(rec * sizeof(double));
    s.state = s.idx + up16(rec * sizeof(int32_t));
    s.total = s.state + up16(sizeof(PcState));
    return s;
}

// (key, idx) <- the better of it and (okey, oidx): the larger key, ties to the lower row index.  A total order, so a
// butterfly of these leaves the same winner in every lane.
static __device__ __forceinline__ void pc_better(double& key, int& idx, double okey, int oidx)
{
    if (okey > key || (okey == key && oidx < idx)) { key = okey; idx = oidx; }
}

// One wave's record for its 64 rows.  unpicked: this lane's row is live and not picked; d its residual.  key = d, or
// -infinity for a NaN (never larger than anything, and still a valid row); trace share max(d, 0), or d itself in the
// start pass (plain).  wave_sum's butterfly adds the shares; lane 0 writes.
static __device__ __forceinline__ void pc_record(bool unpicked, double d, int i, bool plain, int64_t rec, double* __restrict__ pval,
                                                 double* __restrict__ ptr, int32_t* __restrict__ pidx)
{
    double key = -INFINITY;
    int idx = PC_NONE;
    double tr = 0.0;
    if (unpicked) {
        key = (d != d) ? -INFINITY : d;
        idx = i;
        tr = plain ? d : fmax(d, 0.0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double okey = __shfl_xor(key, off, 64);
        const int oidx = __shfl_xor(idx, off, 64);
        pc_better(key, idx, okey, oidx);
    }
    wave_sum(tr);
    if ((threadIdx.x & 63) == 0) { pval[rec] = key; ptr[rec] = tr; pidx[rec] = idx; }
}

// blockIdx.x < ceil(n / 64), 64 threads: d_i = sf2 + sum_e lin[e] x_ie^2, no row picked, the first records
__global__ __launch_bounds__(64)
void k_pc_init(const double* __restrict__ x, int n, int d, double sf2, const double* __restrict__ lin, double* __restrict__ diag,
               int32_t* __restrict__ mark, double* __restrict__ pval, double* __restrict__ ptr, int32_t* __restrict__ pidx)
{
    const int i = blockIdx.x * PC_ROWS + (int)threadIdx.x;
    const bool live = i < n;
    double di = 0.0;
    if (live) {
        double s = 0.0;
        if (lin) {
            for (int e = 0; e < d; ++e) {
                const double v = x[(int64_t)i * d + e];
                s += lin[e] * v * v;
            }
        }
        di = lin ? sf2 + s : sf2;
        diag[i] = di;
        mark[i] = 0;
    }
    pc_record(live, di, i, true, blockIdx.x, pval, ptr, pidx);
}

// Step j of the factorisation for rows blockIdx.x * 64 .. + 63 (header comment).  D: the input dimension as 1, 2 or 0 (run time)
template <int COV, int D>
__global__ __launch_bounds__(256)
void k_pc_column(const double* __restrict__ x, int n, int d, double c, double sf2, const double* __restrict__ lin, double floor_value,
                 int j, const PcState* __restrict__ state, const double* __restrict__ prow, double* __restrict__ lt, int64_t ldl,
                 double* __restrict__ diag, int32_t* __restrict__ mark, double* __restrict__ pval, double* __restrict__ ptr,
                 int32_t* __restrict__ pidx)
{
    __shared__ double sp[PC_CHUNK];
    __shared__ double red[4][PC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * PC_ROWS + lane;
    const bool live = i < n;
    const int p = (int)state->p;
    const double dp = state->dp;
    const bool active = dp > floor_value;           // the same in every thread of the grid; false for a NaN

    double acc = 0.0;
    if (active) {
        for (int t0 = 0; t0 < j; t0 += PC_CHUNK) {
            const int cnt = min(PC_CHUNK, j - t0);
            __syncthreads();
            for (int e = tid; e < cnt; e += 256) sp[e] = prow[t0 + e];
            __syncthreads();
            if (live) {
                // wave w: t0 + w, t0 + w + 4, ..: PC_CHUNK is a multiple of 4, so t = w (mod 4) throughout, ascending
                const double* col = lt + (int64_t)(t0 + wave) * ldl + i;
                int e = wave;
                for (; e + 4 * (PC_UNROLL - 1) < cnt; e += 4 * PC_UNROLL) {
                    double v[PC_UNROLL];
#pragma unroll
                    for (int u = 0; u < PC_UNROLL; ++u) v[u] = col[(int64_t)(4 * u) * ldl];
#pragma unroll
                    for (int u = 0; u < PC_UNROLL; ++u) acc = fma(v[u], sp[e + 4 * u], acc);
                    col += (int64_t)(4 * PC_UNROLL) * ldl;
                }
                for (; e < cnt; e += 4) {
                    acc = fma(col[0], sp[e], acc);
                    col += 4 * ldl;
                }
            }
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;

    bool unpicked = false;
    double di = 0.0;
    if (live) {
        unpicked = mark[i] == 0;
        di = diag[i];
        double* out = lt + (int64_t)j * ldl + i;
        if (active) {
            const double s = sum4(red[0][lane], red[1][lane], red[2][lane], red[3][lane]);
            constexpr int DD = D ? D : MAXD;
            double d2 = 0.0, df0 = 0.0, dot = 0.0;
#pragma unroll
            for (int k = 0; k < DD; ++k) {
                if (D || k < d) {
                    const double xi = x[(int64_t)i * d + k], xp = x[(int64_t)p * d + k];
                    const double df = xi - xp;
                    if (k == 0) df0 = df;
                    d2 += df * df;
                    if (lin) dot += lin[k] * xi * xp;
                }
            }
            const double kv = Cov<COV>::template value<double, D>(d2, df0, c, sf2) + dot;
            const double ci = (kv - s) / sqrt(dp);
            *out = ci;
            if (unpicked) {
                di -= ci * ci;
                diag[i] = di;
            }
        } else {
            *out = 0.0;
        }
        if (i == p) {
            mark[i] = 1;
            diag[i] = -1.0;
            unpicked = false;
        }
    }
    pc_record(unpicked, di, i, false, blockIdx.x, pval, ptr, pidx);
}

// One workgroup of 256 threads, after the records of step j - 1 (or of the start pass, j = 0): trace[j]; for j < m the
// pivot of step j, its residual, the rank count, and prow[t] = L[p][t] for t < j.  Thread t takes records t, t + 256, ..
// in order; then a pairwise tree over the 256 threads (lds_tree's order for the trace, the same pairs for the arg-max).
__global__ __launch_bounds__(256)
void k_pc_pick(int j, int m, int n, int records, const double* __restrict__ pval, const double* __restrict__ ptr,
               const int32_t* __restrict__ pidx, const double* __restrict__ diag, double floor_value, PcState* __restrict__ state,
               int64_t* __restrict__ pivots, double* __restrict__ trace, int64_t* __restrict__ rank, const double* __restrict__ lt,
               int64_t ldl, double* __restrict__ prow)
{
    __shared__ double skey[256];
    __shared__ double str[256];
    __shared__ int sidx[256];
    const int tid = threadIdx.x;
    double key = -INFINITY, tr = 0.0;
    int idx = PC_NONE;
    for (int r = tid; r < records; r += 256) {
        pc_better(key, idx, pval[r], pidx[r]);
        tr += ptr[r];
    }
    skey[tid] = key; sidx[tid] = idx; str[tid] = tr;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half) {
            pc_better(key, idx, skey[tid + half], sidx[tid + half]);
            skey[tid] = key; sidx[tid] = idx;
            str[tid] += str[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) trace[j] = str[0];
    if (j >= m) return;
    // m <= n: at least one row is not picked, so the winner is a row; the clamp only keeps a broken record inside x and lt
    const int p = min(max(sidx[0], 0), n - 1);
    if (tid == 0) {
        const double dp = diag[p];
        state->p = p;
        state->dp = dp;
        pivots[j] = p;
        const int64_t before = j == 0 ? 0 : rank[0];
        rank[0] = before + (dp > floor_value ? 1 : 0);
    }
    for (int t = tid; t < j; t += 256) prow[t] = lt[(int64_t)t * ldl + p];
}

static int pc_run(int cov, const double* x, int64_t n, int d, double ell, double sf2, const double* lin, int64_t m, double floor_value,
                  int64_t* pivots, double* lt, int64_t ldl, double* diag, double* trace, int64_t* rank, char* scratch, hipStream_t st,
                  const char* fn)
{
    const PcScratch lay = pc_scratch(n, m);
    double* prow = reinterpret_cast<double*>(scratch + lay.prow);
    int32_t* mark = reinterpret_cast<int32_t*>(scratch + lay.mark);
    double* pval = reinterpret_cast<double*>(scratch + lay.val);
    double* ptr = reinterpret_cast<double*>(scratch + lay.tr);
    int32_t* pidx = reinterpret_cast<int32_t*>(scratch + lay.idx);
    PcState* state = reinterpret_cast<PcState*>(scratch + lay.state);
    const unsigned records = (unsigned)pc_records(n);
    const double c = cov_scale(cov, ell);

    hipLaunchKernelGGL(k_pc_init, dim3(records), dim3(PC_ROWS), 0, st, x, (int)n, d, sf2, lin, diag, mark, pval, ptr, pidx);
    CIMRGP_LAUNCH_CHECK(fn);
    return with_cov(cov, [&](auto cc) -> int {
        return with_dim(d, [&](auto dd) -> int {
            constexpr int COV = decltype(cc)::value;
            constexpr int D = decltype(dd)::value;
            for (int64_t j = 0; j <= m; ++j) {
                hipLaunchKernelGGL(k_pc_pick, dim3(1), dim3(256), 0, st, (int)j, (int)m, (int)n, (int)records, (const double*)pval,
                                   (const double*)ptr, (const int32_t*)pidx, (const double*)diag, floor_value, state, pivots, trace, rank,
                                   (const double*)lt, ldl, prow);
                CIMRGP_LAUNCH_CHECK(fn);
                if (j == m) break;
                hipLaunchKernelGGL((k_pc_column<COV, D>), dim3(records), dim3(256), 0, st, x, (int)n, d, c, sf2, lin, floor_value, (int)j,
                                   (const PcState*)state, (const double*)prow, lt, ldl, diag, mark, pval, ptr, pidx);
                CIMRGP_LAUNCH_CHECK(fn);
            }
            return 0;
        });
    });
}

}  // namespace

}  // namespace cimrgp

using namespace cimrgp;

extern "C" {

size_t cimrgp_pivoted_cholesky_scratch_bytes(int64_t n, int64_t m)
{
    if (!pc_sizes_ok(n, m)) return 0;
    return pc_scratch(n, m).total;
}

int cimrgp_pivoted_cholesky(int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2, const double* lin_dev,
                            int64_t m, double floor, int64_t* pivots_dev, void* lt_dev, int64_t ldl, double* diag_dev,
                            double* trace_dev, int64_t* rank_dev, void* scratch_dev, size_t scratch_bytes, void* stream)
{
    const char* fn = "cimrgp_pivoted_cholesky";
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(dtype == CIMRGP_F64, fn, "FP32 is not built (the residual's cancellation needs FP64)");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(x_dev && pivots_dev && lt_dev && diag_dev && trace_dev && rank_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), fn, "n must be in [1, 2^31)");
    CIMRGP_REQUIRE(m >= 1 && m <= n, fn, "m must be in [1, n]");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "ell and sf2 must be positive");
    CIMRGP_REQUIRE(floor >= 0.0 && floor <= 1.79769313486231570815e308, fn, "floor must be finite and not negative");
    CIMRGP_REQUIRE(ldl >= n, fn, "leading dimension too small");
    CIMRGP_REQUIRE(aligned16(scratch_dev), fn, "scratch must be 16-byte aligned");
    CIMRGP_REQUIRE(scratch_bytes >= cimrgp_pivoted_cholesky_scratch_bytes(n, m), fn, "scratch too small");
    return pc_run(cov, (const double*)x_dev, n, d, ell, sf2, lin_dev, m, floor, pivots_dev, (double*)lt_dev, ldl, diag_dev, trace_dev,
                  rank_dev, (char*)scratch_dev, stream_of(stream), fn);
}

}  // extern "C"
