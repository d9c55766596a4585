// Device code of the Cholesky factorisation's panel chain: the 64 x 64 diagonal factorisation (nine-wave and
// four-wave forms), the links (panel solve of one sub-block beside the factorisation of the next), the panel
// solves and the update tiles that ride in the chain's launches.  Included by potrf.hip only, which holds the
// host schedule: the whole factorisation stays one translation unit.
// Tile traffic: load_tile64 and gload_tile64 (both read through gpiece), swrite_tile64; products: mma_chunk64 / 32.
#pragma once
#include "common.hpp"
#include "gemm_tile.hpp"

namespace cimrgp {
namespace {

constexpr int SB = 64;   // diagonal sub-block

// 16 bytes in flight between global memory and LDS.  A first-class vector: arrays of HIP's uint4
// struct filled from global memory stay in scratch (the optimiser does not split the struct copy).
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ v4u v4u_zero() { v4u z = {0u, 0u, 0u, 0u}; return z; }

template <typename T> struct Tile64 {
    static constexpr int ROWB  = SB * (int)sizeof(T);   // bytes of 64 k-values per row
    static constexpr int LROW  = ROWB + 16;              // padded LDS row stride
    static constexpr int CPR   = ROWB / 16;              // 16-byte chunks per row
    static constexpr int NSTEP = ROWB / 32;              // slot-steps (4 slots x 8 B) per 64 k
    static constexpr int KPS   = 32 / (int)sizeof(T);    // k values per slot-step
    static constexpr int BYTES = SB * LROW;
};

// mask_chunk for the first-class vector: zero the elements whose k index is >= kvalid
template <typename T> static __device__ __forceinline__ v4u mask_v4u(v4u v, int kfirst, int kvalid)
{
    const uint4 m = mask_chunk<T>(make_uint4(v.x, v.y, v.z, v.w), kfirst, kvalid);
    v4u o = {m.x, m.y, m.z, m.w};
    return o;
}

// Piece (r, c) -- 16 bytes -- of a 64 x kw strip in global memory (row stride ld elements); rows >= mrows and
// columns >= kw read as zero.
template <typename T>
static __device__ __forceinline__ v4u gpiece(const T* src, int64_t ld, int r, int c, int mrows, int kw)
{
    using X = Mx<T>;
    const int kcol = c * X::EPC;
    v4u v = v4u_zero();
    if (r < mrows && kcol < kw) {
        v = *reinterpret_cast<const v4u*>(src + (int64_t)r * ld + kcol);
        if (kcol + X::EPC > kw) v = mask_v4u<T>(v, kcol, kw);
    }
    return v;
}

// Cooperative, coalesced load of a 64 x kw strip (row stride ld elements) into a
// padded LDS tile; rows >= mrows and columns >= kw are zero-filled.
template <typename T, int ROWS = SB>
static __device__ __forceinline__ void load_tile64(unsigned char* dst, const T* __restrict__ src, int64_t ld,
                                                    int mrows, int kw)
{
    using TL = Tile64<T>;
    for (int e = threadIdx.x; e < ROWS * TL::CPR; e += 256) {
        const int r = e / TL::CPR, c = e - r * TL::CPR;
        *reinterpret_cast<v4u*>(dst + r * TL::LROW + c * 16) = gpiece<T>(src, ld, r, c, mrows, kw);
    }
}

// Same strip, split in two halves so the global loads of the next k chunk can be in
// flight (in registers) while the current chunk is multiplied.
template <typename T, int ROWS>
static __device__ __forceinline__ void gload_tile64(v4u (&regs)[ROWS * Tile64<T>::CPR / 256], const T* __restrict__ src,
                                                     int64_t ld, int mrows, int kw)
{
    using TL = Tile64<T>;
#pragma unroll
    for (int p = 0; p < ROWS * TL::CPR / 256; ++p) {
        const int e = threadIdx.x + 256 * p;
        const int r = e / TL::CPR, c = e - r * TL::CPR;
        regs[p] = gpiece<T>(src, ld, r, c, mrows, kw);
    }
}

// NT = the threads that share the tile
template <typename T, int ROWS, int NT = 256>
static __device__ __forceinline__ void swrite_tile64(unsigned char* dst, const v4u (&regs)[ROWS * Tile64<T>::CPR / NT])
{
    using TL = Tile64<T>;
#pragma unroll
    for (int p = 0; p < ROWS * TL::CPR / NT; ++p) {
        const int e = threadIdx.x + NT * p;
        const int r = e / TL::CPR, c = e - r * TL::CPR;
        *reinterpret_cast<v4u*>(dst + r * TL::LROW + c * 16) = regs[p];
    }
}

// acc[ct] += A(16 rows of this wave) * B(rows 16 ct ..)^T over one 64-wide k chunk.
template <typename T, bool TRI>
static __device__ __forceinline__ void mma_chunk64(typename Mx<T>::acc_t (&acc)[4], const unsigned char* as,
                                                    const unsigned char* bs, int wave, int lane)
{
    using X = Mx<T>;
    using TL = Tile64<T>;
    const int frow = lane & 15, fslot = lane >> 4;
    const unsigned char* pa = as + (wave * 16 + frow) * TL::LROW + fslot * 8;
    const unsigned char* pb = bs + frow * TL::LROW + fslot * 8;
    // unrolled by 4 only: fully unrolled, the 80 fragment reads of a chunk are all issued up front and
    // hold 160 registers (the four-wave kernels must stay within 256 to fit beside an update workgroup)
#pragma unroll 4
    for (int s = 0; s < TL::NSTEP; ++s) {
        const uint2 a = *reinterpret_cast<const uint2*>(pa + s * 32);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            // TRI: B is lower triangular (B[j][k] = 0 for k > j): column tile ct needs k <= 16 ct + 15
            if (!TRI || (s * TL::KPS <= 16 * ct + 15)) {
                const uint2 b = *reinterpret_cast<const uint2*>(pb + ct * 16 * TL::LROW + s * 32);
                acc[ct] = X::mma(a, b, acc[ct]);
            }
        }
    }
}

// 32-row variant: wave = (rt = row tile 0/1, ch = column half 0/1): 16 rows x 32 columns.
template <typename T, bool TRI>
static __device__ __forceinline__ void mma_chunk32(typename Mx<T>::acc_t (&acc)[2], const unsigned char* as,
                                                    const unsigned char* bs, int rt, int ch, int lane)
{
    using X = Mx<T>;
    using TL = Tile64<T>;
    const int frow = lane & 15, fslot = lane >> 4;
    const unsigned char* pa = as + (rt * 16 + frow) * TL::LROW + fslot * 8;
    const unsigned char* pb = bs + (ch * 32 + frow) * TL::LROW + fslot * 8;
#pragma unroll
    for (int s = 0; s < TL::NSTEP; ++s) {
        // TRI: column tile ct = 2 ch + c needs k <= 16 ct + 15; ch is run-time (wave-uniform)
        if (!TRI || (s * TL::KPS <= 16 * (2 * ch + 1) + 15)) {
            const uint2 a = *reinterpret_cast<const uint2*>(pa + s * 32);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (!TRI || (s * TL::KPS <= 16 * (2 * ch + c) + 15)) {
                    const uint2 b = *reinterpret_cast<const uint2*>(pb + c * 16 * TL::LROW + s * 32);
                    acc[c] = X::mma(a, b, acc[c]);
                }
            }
        }
    }
}

// Wave-local broadcast of lane `src`'s value (src wave-uniform): v_readlane, no LDS.
static __device__ __forceinline__ double bcast_lane(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
static __device__ __forceinline__ float bcast_lane(float v, int src)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

template <typename T> static __device__ __forceinline__ T rsqrt_refined(T d);
template <> __device__ __forceinline__ double rsqrt_refined<double>(double d)
{
    double r = __builtin_amdgcn_rsq(d);          // ~2^-26; two Newton steps -> full f64
    {
        const double e0 = fma(-d * r, r, 1.0);
        r = fma(0.5 * r, e0, r);
    }
    const double e = fma(-d * r, r, 1.0);       // one Newton step: full f64 accuracy
    return fma(0.5 * r, e, r);
}
template <> __device__ __forceinline__ float rsqrt_refined<float>(float d)
{
    float r = rsqrtf(d);
    const float e = fmaf(-d * r, r, 1.0f);
    return fmaf(0.5f * r, e, r);
}

// hardware reciprocal estimate (v_rcp_f64 / v_rcp_f32): the pivot recurrence refines it itself
static __device__ __forceinline__ double rcp_seed(double d) { return __builtin_amdgcn_rcp(d); }
static __device__ __forceinline__ float rcp_seed(float d) { return __builtin_amdgcn_rcpf(d); }

// ---------------------------------------------------------------------------
// Riders (round 3).  The launches of a panel's chain are latency-bound: one workgroup factors a 64 x 64
// block for 17-31 us while the 30-250 panel-solve workgroups beside it are gone after ~10 us and most
// compute units idle.  In the one-queue sweeps (small matrices, batches, the tail of a large
// factorisation) the trailing updates therefore no longer get launches of their own: they are cut into
// 64 x 64 tiles (gemm_tile, W = 2) that ride as extra workgroups of the chain's launches -- the update by
// the PREVIOUS panel in the launches of this panel's chain, and the update of the next panel's columns by
// this panel sub-block by sub-block (K = 64) as soon as a sub-block is final, so that the next chain
// never waits for a "head" update either (fused_sweep has the schedule).  One queue, no inter-queue
// signal, and the chain's workgroup 0 is dispatched first in its launch.
// ---------------------------------------------------------------------------
template <typename T> struct RiderJob {
    T* c; const T* a; const T* b;      // C[m x n] -= A[m x k] B[n x k]^T
    int64_t ldc, lda, ldb;
    int m, n, k;
    int lower;                          // 1: lower-triangular grid of tiles (square C), 0: rectangular
    int tiles_n;                        // tiles per row of the rectangular grid
    int first, count;                   // this launch runs tiles [first, first + count) of the job
    int skip00;                         // tile (0, 0) is left alone: the chain's workgroup 0 owns it
    int rows_job;                       // 1: c and a are carried rows (batch stride sb), 0: the matrix (stride sk)
};
constexpr int MAX_RIDER_JOBS = 6;
template <typename T> struct Riders {
    RiderJob<T> job[MAX_RIDER_JOBS];
    int njobs;
    int total;                          // sum of the jobs' counts = extra workgroups of the launch
};
template <typename T> static Riders<T> no_riders() { Riders<T> r; r.njobs = 0; r.total = 0; return r; }

constexpr int RIDER_LDS = 4 * 64 * (128 + 16);      // gemm_tile<.., W = 2>: 2 stages x 2 operands x 64 rows x 144 bytes
// LDS of a chain kernel that also hosts riders: the larger of the panel solve's area and a rider's (f32: the rider's)
template <typename T> struct ChainLds {
    static constexpr int TRSM = (2 * 32 + 64) * (64 * (int)sizeof(T) + 16);          // = TrsmLds<T>::BYTES
    static constexpr int BYTES = TRSM > RIDER_LDS ? TRSM : RIDER_LDS;
};

// Workgroup number r (0 <= r < rd.total) of a launch's riders; the first 256 threads of the workgroup.
template <typename T>
static __device__ __forceinline__ void run_rider(unsigned char* smem, const Riders<T>& rd, int r, int64_t sk, int64_t sb)
{
    int j = 0;
    while (j + 1 < rd.njobs && r >= rd.job[j].count) { r -= rd.job[j].count; ++j; }       // uniform
    const RiderJob<T>& jb = rd.job[j];
    const int id = jb.first + r;
    int ti, tj;
    if (jb.lower) {
        ti = (int)((sqrtf(8.0f * (float)id + 1.0f) - 1.0f) * 0.5f);
        while (ti * (ti + 1) / 2 > id) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
        tj = id - ti * (ti + 1) / 2;
    } else {
        ti = id / jb.tiles_n;
        tj = id - ti * jb.tiles_n;
    }
    if (jb.skip00 && ti == 0 && tj == 0) return;
    const int64_t off_ca = (int64_t)blockIdx.y * (jb.rows_job ? sb : sk);
    T* c = jb.c + off_ca;
    const T* a = jb.a + off_ca;
    const T* b = jb.b + (int64_t)blockIdx.y * sk;
    constexpr int BKE = 128 / (int)sizeof(T);
    const bool interior = (ti + 1) * 64 <= jb.m && (tj + 1) * 64 <= jb.n && (jb.k % BKE) == 0;
    if (jb.lower) {
        if (interior) gemm_tile<T, true, false, 2>(smem, c, jb.ldc, a, jb.lda, b, jb.ldb, jb.m, jb.n, jb.k, ti, tj);
        else          gemm_tile<T, true, true, 2>(smem, c, jb.ldc, a, jb.lda, b, jb.ldb, jb.m, jb.n, jb.k, ti, tj);
    } else {
        if (interior) gemm_tile<T, false, false, 2>(smem, c, jb.ldc, a, jb.lda, b, jb.ldb, jb.m, jb.n, jb.k, ti, tj);
        else          gemm_tile<T, false, true, 2>(smem, c, jb.ldc, a, jb.lda, b, jb.ldb, jb.m, jb.n, jb.k, ti, tj);
    }
}

// ---------------------------------------------------------------------------
// Diagonal 64x64 sub-block of a panel (left-looking inside the panel):
//   S = A_ss - Lrow Lrow^T        Lrow = the kprev panel columns left of the
//                                 block, already final (MFMA, K = kprev <= 192)
//   S = L L^T  in place, inv slab = L^-1 (lower; zero elsewhere).
// Factor and inverse advance together on the unscaled Schur complement S and the
// unscaled inverse Mi: column j of L is S[:,j] r_j and row j of L^-1 is
// Mi[j,:] r_j, r_j = 1/sqrt(S[j][j]); the row operations that reduce S are
// applied to Mi.
// ---------------------------------------------------------------------------
// (lds_barrier, lds_settle: common.hpp)
#define CHAIN_SETPRIO() __builtin_amdgcn_s_setprio(3)
// S and Mi are held as ONE combined 64x64 array A:
//     A[i][k] = S[i][k]   for k <= i   (Schur complement, lower triangle)
//     A[i][k] = Mi[k][i]  for k >  i   (unscaled inverse, stored transposed in the upper triangle)
// At pivot j everything needed is column j of A: A[i][j] is S[i][j] for i >= j and
// Mi[j][i] for i < j, and
//     A[i][k] -= (A[k][j] r) * h_i   for every k > j,    r = 1/sqrt(A[j][j]),
//     h_i = L[i][j] = A[i][j] r (i > j),  L^-1[j][i] = A[i][j] r (i < j),  r (i = j, from 0)
// covers the Schur update, the inverse update and the birth of column j of Mi in one
// formula (for j < i < k it touches a not-yet-born Mi slot, which is reset at pivot i).
constexpr int DG_TW = 8;              // tile waves of the diagonal kernel (two 16x16 tiles each)
constexpr int DG_NW = DG_TW + 1;      // + the pivot wave
constexpr int DG_NT = 64 * DG_NW;

// One 16x16x4 matrix-core step (K = 4 = the pivots of one block).
static __device__ __forceinline__ Mx<double>::acc_t mfma_k4(double a, double b, Mx<double>::acc_t c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
static __device__ __forceinline__ Mx<float>::acc_t mfma_k4(float a, float b, Mx<float>::acc_t c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Version 3 of the diagonal kernel.  The combined array A (see above) lives in MATRIX-CORE
// ACCUMULATOR layout in eight "tile" waves: wave g < 8 owns the two 16x16 tiles (row tile g >> 1,
// column tiles 2 (g & 1) + {0, 1}).  A ninth wave, the pivot wave, works in "lane = row" layout
// on four columns at a time.  Per block p of BC = 4 pivots, ONE barrier:
//   pivot wave   takes block p's columns (gathered by the tile waves one iteration earlier, i.e.
//                updated through block p-2), applies block p-1's rank-4 update to them itself
//                (16 FMAs per lane, coefficients by v_readlane from its own registers), eliminates
//                the 4 pivots among themselves (wave-local broadcasts, 4 dependent rsqrt/scale
//                steps) and publishes the rank-4 update's two operands (64 x 4 each);
//   tile waves   meanwhile apply block p-1's update to their tiles with one matrix-core
//                instruction per tile, then gather block p+1's columns for the pivot wave.
// The pivot-time columns, kept for all 64 pivots, and the 64 reciprocal roots ARE the result:
// L[i][j] = cs[i][j] r_j (i >= j), L^-1[j][i] = cs[i][j] r_j (i < j), L^-1[j][j] = r_j.
// (Version 1 kept A in "lane = row" registers in all waves and applied the rank-4 update with
// scalar FMAs whose per-column coefficients every wave read as LDS broadcasts: 2 MB of LDS
// return traffic per block, 1.1 us per 4 pivots of which the pivots themselves were 0.24 us.)
// One block of BC = 4 pivots in the pivot wave (lane = row i), shared by the nine-wave and the four-wave
// factorisation: takes the block's columns `nx` as gathered (updated through block p-3; rows of blocks p-2 and
// p-1 gathered as ZERO: their slots restart there), applies the rank-4 updates of blocks p-2 and p-1 to them
// itself, eliminates the 4 pivots and publishes the rank-4 update's two operands (hs_row: this row's left operand, UNMASKED --
// the tile waves zero the three entries of a block's own rows that lie below their pivots; cs: the
// pivot-time columns, kept for all 64 pivots).
//
// Round 4: this wave is ISSUE-bound, not latency-bound.  A lone wave issues one instruction per ~5 clocks
// (phase stamps, HISTORY.md round 4: 4 pivots = 750-790 clocks with an 11-deep dependent chain per pivot and just the
// same with a 5-deep one), and an iteration of rounds 1-3 was ~300 instructions of this wave against ~500
// clocks of the tile waves' work.  So everything that is not the recurrence left the loop:
//   * the recurrence needs -A[i][j] / d only: a reciprocal (seed + three fused steps, x0 (1 + e)(1 + e^2)),
//     no root.  The reciprocal roots -- which only scale the OUTPUT -- and the first non-positive pivot are
//     taken after the loop from the pivots themselves, d_j = cs[j][j] (a pivot-time column is final from
//     its own pivot on): diag_roots;
//   * row j itself takes the generic -A[j][j] / d = -1 instead of -1/d, i.e. column i of the unscaled
//     inverse is kept scaled by d_i (its birth needs no division and no select; the recurrence of an
//     inverse column is linear in it; the epilogue multiplies by r_i^2): no special case for lane j;
//   * "restart from zero" of a slot is one select on the high word (tiny_if): as an addend a double
//     below 2^-1042 is zero.
template <typename T> static __device__ __forceinline__ T tiny_if(T v, bool c);
template <> __device__ __forceinline__ double tiny_if<double>(double v, bool c)
{
    return __hiloint2double(c ? 0 : __double2hiint(v), __double2loint(v));
}
template <> __device__ __forceinline__ float tiny_if<float>(float v, bool c) { return c ? 0.0f : v; }

template <typename T>
static __device__ __forceinline__ void pivot_block(int p, T (&nx)[4], T (&cv)[4], T (&hsr)[4], T (&hsr2)[4],
                                                    T (&sm1)[4][4], T (&sm2)[4][4],
                                                    T* __restrict__ hs_row, T* __restrict__ cs, int i)
{
    constexpr int LS = SB + 2;
    constexpr int BC = 4;
    constexpr int NP = SB / BC;
    const int j0 = BC * p;
    // The 4 x 4 coefficients of an earlier block's rank-4 update = its pivot-time columns at the rows of block p,
    // published in `cs` by THIS wave: sm1 (block p-1) and sm2 (block p-2) were requested at
    // the end of the previous block, behind its publishing stores and ahead of its barrier (below).  One chain of fused
    // operations per column (fewest instructions).
    // the gathered columns carry the updates through block p-3: two self-updates here.
    // Rows of block p-2 and p-1 arrive as zero (their slots restart there); a row of block p-1 takes nothing from
    // block p-2 (not born yet: reset between the two updates).
    if (p > 1) {
        const bool rows_prev = (unsigned)(i - (j0 - BC)) < (unsigned)BC;
#pragma unroll
        for (int t2 = 0; t2 < BC; ++t2) {
            T u = nx[t2];
#pragma unroll
            for (int t = 0; t < BC; ++t) u = fma(hsr2[t], sm2[t2][t], u);
            nx[t2] = tiny_if<T>(u, rows_prev);
        }
    }
    if (p > 0) {
#pragma unroll
        for (int t2 = 0; t2 < BC; ++t2) {
            T u = nx[t2];
#pragma unroll
            for (int t = 0; t < BC; ++t) u = fma(hsr[t], sm1[t2][t], u);
            nx[t2] = u;
        }
    }
#pragma unroll
    for (int t = 0; t < BC; ++t) cv[t] = nx[t];
    T nh[BC];
#pragma unroll
    for (int t = 0; t < BC; ++t) {
        const int j = j0 + t;
        const T d = bcast_lane(cv[t], j);
        const T x0 = rcp_seed(d);
        const T e = fma(-d, x0, (T)1);
        const T sx0 = -cv[t] * x0;
        const T sx1 = fma(sx0, e, sx0);
        nh[t] = fma(sx1, e * e, sx1);                                // -A[i][j] / d  (row j: -1)
#pragma unroll
        for (int t2 = t + 1; t2 < BC; ++t2) {
            const T ak = bcast_lane(cv[t], j0 + t2);                // A[k][j] at pivot time
            cv[t2] = fma(nh[t], ak, tiny_if<T>(cv[t2], i == j));    // row j: its slots right of the pivot are born here
        }
    }
    T* cp = &cs[i * LS + j0];
#pragma unroll
    for (int t = 0; t < BC; ++t) {
        hs_row[t] = nh[t];
        cp[t] = cv[t];
    }
    // Round 5: the NEXT block's coefficients are requested here, behind the publishing stores and ahead of the barrier.
    // (1) They are this wave's own words (rows j0+4 .. j0+7 of the columns just published and of the block before), so
    //     nothing is waited for that is not there; behind the barrier only the gathered columns remain to be read.
    // (2) The barrier's wait for these LOADS is what makes the stores above visible to the tile waves that read `hs`
    //     and `cs` right behind the barrier: the LDS executes a wave's accesses in order, so the loads' data returns
    //     only after the stores have been performed -- the wait for a store's lgkmcnt alone does not imply that
    //     (lds_settle in common.hpp has the measurement).  The last block settles on its last word instead.
    if (p + 1 < NP) {
        const T* sp = &cs[(j0 + BC) * LS + j0];
#pragma unroll
        for (int t2 = 0; t2 < BC; ++t2)
#pragma unroll
            for (int t = 0; t < BC; ++t) sm1[t2][t] = sp[t2 * LS + t];
        if (p > 0) {
#pragma unroll
            for (int t2 = 0; t2 < BC; ++t2)
#pragma unroll
                for (int t = 0; t < BC; ++t) sm2[t2][t] = sp[t2 * LS + t - BC];
        }
    } else {
        lds_settle(&cp[BC - 1]);
    }
    // this wave's own copies of the left operand, for the next blocks' self-updates: a row of THIS block takes
    // nothing from the pivots above it (its slots right of the block are born at its own pivot)
#pragma unroll
    for (int t = 0; t < BC; ++t) hsr2[t] = hsr[t];
    const unsigned u = (unsigned)(i - j0);
    hsr[0] = tiny_if<T>(nh[0], u - 1u < 3u);
    hsr[1] = tiny_if<T>(nh[1], u - 2u < 2u);
    hsr[2] = tiny_if<T>(nh[2], u == 3u);
    hsr[3] = nh[3];
}

// After the pivot loop (all waves past a barrier): the reciprocal roots r_j = 1 / sqrt(d_j) from the pivots
// d_j = cs[j][j], and the first non-positive pivot among the block's w columns.  One wave, lane = j.
template <typename T>
static __device__ __forceinline__ void diag_roots(const T* __restrict__ cs, T* __restrict__ rall, int lane, int w,
                                                   int32_t* info, int col_base)
{
    constexpr int LS = SB + 2;
    const T d = cs[lane * LS + lane];
    rall[lane] = rsqrt_refined<T>(d);
    lds_settle(&rall[lane]);                 // every wave reads the roots right behind the next barrier
    const unsigned long long badmask = __ballot(lane < w && !(d > (T)0));
    if (badmask != 0ull && lane == 0) atomicCAS(info, 0, col_base + __ffsll((long long)badmask));
}

// The factorisation proper, shared by all four chain kernels.  On entry `cs` holds the Schur complement S
// (lower triangle, identity padding beyond w, zeros above the diagonal) and every wave has passed a barrier
// behind its writer; `pcol`, `hs`, `rall` are LDS areas nobody reads any more.  Writes L into D (lower) and
// L^-1 into `inv`.
//   tw >= 0   tile wave number tw of NTW: owns the 16 x 16 tiles t = tw + NTW k of the combined array
//             (t = 4 row-tile + column-tile) in matrix-core accumulator layout;
//   pivot     the pivot wave (pivot_block);
//   neither   keeps the barriers only.
// Round 4: WHICH SIMD the pivot wave shares matters more than how many tile waves there are.  The vector ALU
// of a SIMD issues one wave-wide instruction per 4 clocks whatever wave it comes from, and the pivot wave's
// ~140 instructions per block of 4 pivots are the critical path: with two tile waves on its SIMD (rounds 1-3:
// nine waves, waves 0 / 4 / 8 on SIMD 0) an iteration took the SUM of the pivot wave's and the tile waves'
// issue time (HISTORY.md, 200 launches back to back: 13.5 us per kernel; tile waves idle 10.1;
// pivot wave idle 7.5).  So the nine-wave kernels leave waves 0 and 4 idle in the loop and deal the sixteen
// tiles to the six waves of the other three SIMDs (nine_tile_wave), the four-wave kernels keep three tile
// waves beside a pivot wave with a SIMD of its own.
// Tile ownership: a tile wave owns tiles of ONE 16-column block BCOL (two in the four-wave form's last wave), rows
// BR0 .. BR0 + NB - 1.  All its tiles then share the right operand, are final together (one uniform early-out per
// block of pivots), and its step is straight-line code: every operand is requested before the first multiply
// (with the sixteen tiles dealt round-robin, each tile sat behind its own branches and paid its own LDS round
// trip: 240 clocks per tile, 14.3 us per kernel with the pivot wave idle against 7.5 for two tiles per wave).
// Each role runs its OWN copy of the pivot loop (same number of barriers): with the roles told apart inside one
// loop the compiler moved the accumulators between per-branch register assignments every iteration.
//   nine-wave kernels (6 tile waves): column 3: rows 0-1 | 2-3, column 2: rows 0-1 | 2-3, column 1: all, column 0: all
//   four-wave kernels (3 tile waves): column 3 | column 2 | columns 1 and 0
template <typename T, int NB, int BCOL, int BR0>
struct TileGroup {
    using X = Mx<T>;
    using acc_t = typename X::acc_t;
    static constexpr int LS = SB + 2;
    static constexpr int BC = 4;
    static constexpr int NP = SB / BC;
    acc_t acc[NB > 0 ? NB : 1];
    __device__ __forceinline__ void load(const T* cs, int lane)
    {
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[k][r] = cs[((BR0 + k) * 16 + X::crow(lane, r)) * LS + BCOL * 16 + (lane & 15)];
    }
    // The gather of block p+2 for the pivot wave, THEN block p's rank-4 update of the group's tiles: the columns leave
    // with the updates through block p-1 and the pivot wave applies two blocks itself (its coefficients are in
    // registers by then: pivot_block).
    // Why this order (rounds 4 and 5; HISTORY.md).  With the gather BEHIND the multiplies --
    // rounds 1-3 -- FP32 factorisations beside a running FP32 update came out wrong in 1.7-3 % of the runs, always in
    // the last rows of a block's last columns.  Round 4 blamed matrix-core results landing late and moved the gather
    // ahead; round 5 found what it was: the gathering wave's LAST one or two ds_write instructions -- issued right
    // ahead of `s_waitcnt lgkmcnt(0); s_barrier` -- were not yet in the LDS array when the pivot wave read their
    // words right behind the barrier: it read, bit for bit, what the words held two blocks earlier.  1024 idle cycles
    // between the multiplies and the stores changed nothing (the matrix cores were never late); reading the last
    // stored word back ahead of the barrier cured it (0 of 1999 runs against 60 of 1999).  The LDS executes one wave's
    // accesses in issue order, so a LOAD's returned data proves the wave's earlier stores performed; a store's own
    // lgkmcnt does not prove them visible to another wave.  Here the operand loads below ARE that proof: they are issued
    // behind the gather's stores (the compiler-only fence keeps them there) and the multiplies need their data, so the
    // stores have been performed long before this wave reaches the barrier -- by construction, not by timing.
    // (The same read-back behind the multiplies is correct too and one self-update shorter in the pivot wave, but puts
    // the load's round trip on the tile wave's path: 11.5 / 14.6 us per kernel against 10.7 / 12.3 in this order:
    // profiles/r05_chain_kernels.txt, HISTORY.md.)
    //   right operand = the pivot-time columns at this column block's rows (zero for columns that are final),
    //   left operand per tile = the pivot wave's -A[i][j] / d (a row of the block takes nothing from the pivots
    //   above it: the pivot wave publishes unmasked),
    //   rows of the block: their slots right of it restart from 0 (the one tile concerned: a uniform branch
    //   ahead of the operand reads, so that no join sits between the reads and the multiplies).
    // (no __restrict__ on these: `hs` and `cs` are rewritten by the PIVOT wave between the barriers, at addresses
    // that repeat every second block -- a tile wave that only reads them must not be told they are its own)
    __device__ __forceinline__ void step(int p, const T* hs, const T* cs, T* pcol, int lane)
    {
        if (NB == 0) return;
        const int j0 = BC * p, bc0 = j0 >> 4, jb = j0 & 15;
        if (BCOL < bc0) return;                                   // uniform: every column of the group is final
        const int fcol = lane & 15, fk = lane >> 4;
        const int col = BCOL * 16 + fcol;
        const int g0 = j0 + 2 * BC, gbc = g0 >> 4, gjb = g0 & 15;   // block p+2
        if (p + 2 < NP && BCOL == gbc && fcol >= gjb && fcol < gjb + BC) {
            T* pc = pcol + ((p & 1) * SB) * BC + (fcol - gjb);
#pragma unroll
            for (int k = 0; k < NB; ++k)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // rows of blocks p and p+1 restart from zero in these columns (pivot_block adds to what it is given)
                    const int grow = (BR0 + k) * 16 + X::crow(lane, r);
                    pc[grow * BC] = (grow >= j0 && grow < g0) ? (T)0 : acc[k][r];
                }
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);      // compiler only: the operand loads below stay BEHIND the gather's stores
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (BR0 + k == bc0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rin = X::crow(lane, r);
                    if (rin >= jb && rin < jb + BC && col >= j0 + BC) acc[k][r] = (T)0;
                }
            }
        const T* hsp = hs + ((p & 1) * SB) * BC + fk;
        T bf = cs[col * LS + j0 + fk];
        T af[NB > 0 ? NB : 1];
#pragma unroll
        for (int k = 0; k < NB; ++k) af[k] = hsp[((BR0 + k) * 16 + fcol) * BC];
        if (col < j0 + BC) bf = (T)0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int arow = (BR0 + k) * 16 + fcol;
            if (arow > j0 + fk && arow < j0 + BC) af[k] = (T)0;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = mfma_k4(af[k], bf, acc[k]);
    }
};

// one tile wave's whole pivot loop (two groups; the second may be empty)
template <typename T, int NB, int BCOL, int BR0, int NB2 = 0, int BCOL2 = 0, int BR02 = 0>
static __device__ __forceinline__ void tile_wave_loop(const T* hs, const T* cs, T* pcol, int lane)
{
    TileGroup<T, NB, BCOL, BR0> ga;
    TileGroup<T, NB2, BCOL2, BR02> gb;
    ga.load(cs, lane);
    if (NB2 > 0) gb.load(cs, lane);
    lds_barrier();                                   // every wave has taken its share of S: cs may be overwritten
    for (int p = 0; p < SB / 4; ++p) {
        lds_barrier();
        ga.step(p, hs, cs, pcol, lane);
        if (NB2 > 0) gb.step(p, hs, cs, pcol, lane);
    }
}

template <typename T, int NTW, int NT>
static __device__ __forceinline__ void diag_tail_lds(int tw, bool pivot, T* __restrict__ pcol, T* __restrict__ hs, T* __restrict__ cs,
                                                      T* __restrict__ rall, T* __restrict__ D, int64_t ld,
                                                      int w, T* __restrict__ inv, int32_t* info, int col_base)
{
    static_assert(NTW == 6 || NTW == 3, "tile ownership below");
    constexpr int LS = SB + 2;       // even pitch: a row's 4 block columns are one 16-byte-aligned pair of stores
    constexpr int BC = 4;
    constexpr int NP = SB / BC;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane;
    if (pivot) {
        // ---- pivot wave: the recurrence and nothing else
        T cv[BC], hsr[BC], hsr2[BC];                 // this row's block columns, left operands of the last two blocks
        T sm1[BC][BC], sm2[BC][BC];                  // coefficients of the self-updates, requested one block ahead (pivot_block)
#pragma unroll
        for (int t = 0; t < BC; ++t) {
            cv[t] = (T)0; hsr[t] = (T)0; hsr2[t] = (T)0;
#pragma unroll
            for (int t2 = 0; t2 < BC; ++t2) { sm1[t][t2] = (T)0; sm2[t][t2] = (T)0; }
        }
        T first[3][BC];                              // blocks 0, 1 and 2 straight from S (zero above the diagonal)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int t = 0; t < BC; ++t) first[b][t] = cs[i * LS + b * BC + t];
        lds_barrier();                               // every wave has taken its share of S: cs may be overwritten
        for (int p = 0; p < NP; ++p) {
            T nx[BC];
            if (p < 3) {
#pragma unroll
                for (int t = 0; t < BC; ++t) nx[t] = (p == 0) ? first[0][t] : (p == 1) ? first[1][t] : first[2][t];
            } else {
                // this row's share of block p as gathered (two 16-byte reads, in flight during the FMAs below)
                const T* gp = &pcol[((p & 1) * SB + i) * BC];
#pragma unroll
                for (int t = 0; t < BC; ++t) nx[t] = gp[t];
            }
            pivot_block<T>(p, nx, cv, hsr, hsr2, sm1, sm2, &hs[((p & 1) * SB + i) * BC], cs, i);
            lds_barrier();
        }
    } else if (tw < 0) {
        lds_barrier();
        for (int p = 0; p < NP; ++p) lds_barrier();
    } else if (NTW == 6) {
        if (tw == 0)      tile_wave_loop<T, 2, 3, 0>(hs, cs, pcol, lane);
        else if (tw == 1) tile_wave_loop<T, 2, 3, 2>(hs, cs, pcol, lane);
        else if (tw == 2) tile_wave_loop<T, 2, 2, 0>(hs, cs, pcol, lane);
        else if (tw == 3) tile_wave_loop<T, 2, 2, 2>(hs, cs, pcol, lane);
        else if (tw == 4) tile_wave_loop<T, 4, 1, 0>(hs, cs, pcol, lane);
        else              tile_wave_loop<T, 4, 0, 0>(hs, cs, pcol, lane);
    } else {
        if (tw == 0)      tile_wave_loop<T, 4, 3, 0>(hs, cs, pcol, lane);
        else if (tw == 1) tile_wave_loop<T, 4, 2, 0>(hs, cs, pcol, lane);
        else              tile_wave_loop<T, 4, 1, 0, 4, 0, 0>(hs, cs, pcol, lane);
    }
    __syncthreads();
    if (tid < 64) diag_roots<T>(cs, rall, lane, w, info, col_base);
    __syncthreads();
    for (int e = tid; e < SB * SB; e += NT) {
        const int r = e >> 6, c = e & 63;
        if (r < w && c <= r) D[(int64_t)r * ld + c] = cs[r * LS + c] * rall[c];
        T v = (T)0;
        if (r < w && c < r) v = cs[c * LS + r] * rall[r] * (rall[c] * rall[c]);      // inverse column c is kept scaled by d_c
        if (r < w && c == r) v = rall[r];
        inv[e] = v;
    }
}

// Nine-wave kernels: wave 8 is the pivot wave; it shares SIMD 0 with waves 0 and 4 (waves of a workgroup are
// dealt to the four SIMDs round-robin: measured in round 4, HISTORY.md), which therefore own nothing in the
// pivot loop; tile wave numbers 0..5 go to waves 1, 2, 3, 5, 6, 7.
constexpr int NINE_TW = 6;
static __device__ __forceinline__ int nine_tile_wave(int g) { return ((g & 3) == 0) ? -1 : (g < 4 ? g - 1 : g - 2); }

// Entry of the nine-wave kernels: the eight tile waves hold S in accumulator layout (wave g: row tile
// (g >> 1) & 3, column tiles 2 (g & 1) + {0, 1}) from their left-looking products; it goes to `cs` (dead on
// entry), and behind one barrier -- after which `pcol`, `hs`, `rall` must be dead too -- the pivot loop runs
// with the roles above.
template <typename T>
static __device__ __forceinline__ void diag_tail(typename Mx<T>::acc_t (&acc)[2], T* __restrict__ pcol, T* __restrict__ hs,
                                                  T* __restrict__ cs, T* __restrict__ rall, T* __restrict__ D, int64_t ld,
                                                  int w, T* __restrict__ inv, int32_t* info, int col_base)
{
    using X = Mx<T>;
    constexpr int LS = SB + 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave id: provably uniform
    if (g < DG_TW) {
        const int br = (g >> 1) & 3, ch = g & 1;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cs[(br * 16 + X::crow(lane, r)) * LS + (2 * ch + c) * 16 + (lane & 15)] = acc[c][r];
        lds_settle(&cs[(br * 16 + X::crow(lane, 3)) * LS + (2 * ch + 1) * 16 + (lane & 15)]);
    }
    lds_barrier();
    diag_tail_lds<T, NINE_TW, DG_NT>(nine_tile_wave(g), g == DG_TW, pcol, hs, cs, rall, D, ld, w, inv, info, col_base);
}

// LDS of the factorisation proper, in bytes: pivot columns (cs), gathered columns and left operand
// (double buffered), reciprocal roots.
template <typename T> struct DiagLds {
    static constexpr int CS   = SB * (SB + 2) * (int)sizeof(T);
    static constexpr int PCOL = 2 * SB * 4 * (int)sizeof(T);
    static constexpr int RALL = SB * (int)sizeof(T);
};

template <typename T>
__global__ __launch_bounds__(DG_NT)
void k_diag64(T* __restrict__ D, int64_t ld, int w, const T* __restrict__ Lrow, int kprev,
              T* __restrict__ inv, int32_t* info, int col_base, int64_t sk, int64_t sws, int64_t sb, Riders<T> rd)
{
    static_assert(Tile64<T>::BYTES <= RIDER_LDS, "the prologue chunk and a rider's tiles share one LDS area");
    __shared__ __attribute__((aligned(16))) unsigned char chunk[RIDER_LDS];           // Lrow chunk of the prologue / a rider's tiles
    if (blockIdx.x != 0) {                           // riders: update tiles in the shadow of the pivot loop
        if (threadIdx.x >= 256) return;
        run_rider<T>(chunk, rd, (int)blockIdx.x - 1, sk, sb);
        return;
    }
    // batch of independent factorisations (blocks of one layer): blockIdx.y selects the matrix
    D += (int64_t)blockIdx.y * sk;
    Lrow += (int64_t)blockIdx.y * sk;
    inv += (int64_t)blockIdx.y * sws;
    info += blockIdx.y;
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    constexpr int TT = 64 * DG_TW;                                            // threads of the tile waves
    static_assert(DG_TW == 8 && DG_NW == 9, "tile ownership below assumes 8 tile waves + 1 pivot wave");
    __shared__ __attribute__((aligned(16))) unsigned char pcol_[DiagLds<T>::PCOL];   // gathered pivot columns, double buffered
    __shared__ __attribute__((aligned(16))) unsigned char hs_[DiagLds<T>::PCOL];     // left operand (per row), double buffered
    __shared__ __attribute__((aligned(16))) unsigned char cs_[DiagLds<T>::CS];       // right operand = pivot-time columns, kept
    __shared__ __attribute__((aligned(16))) unsigned char rall_[DiagLds<T>::RALL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave id: provably uniform
    const bool tile_wave = g < DG_TW;
    const int br = (g >> 1) & 3, ch = g & 1;
    const int fcol = lane & 15;
    // latency-bound chain running next to MFMA-bound update workgroups: win issue arbitration
    CHAIN_SETPRIO();

    // the block's own elements are requested first (they depend on nothing), so that their round
    // trip overlaps the left-looking update below instead of following it
    T dval[2][4];
    if (tile_wave) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                dval[c][r] = (row < w && col <= row) ? D[(int64_t)row * ld + col] : (T)0;
            }
    }
    // S = A_ss - Lrow Lrow^T, straight into the accumulator layout
    acc_t pacc[2];
    pacc[0] = acc_zero<T>();
    pacc[1] = acc_zero<T>();
    if (kprev > 0) {
        // kprev <= 192: all (up to three) 64-column chunks of Lrow are requested at once, so only
        // one global round trip is exposed; each then goes registers -> LDS -> matrix cores
        constexpr int NR = SB * TL::CPR / TT;         // 16-byte pieces per thread and chunk
        constexpr int MAXC = (CIMRGP_NB - SB) / SB;
        uint4 regs[MAXC][NR];
        if (tile_wave) {
#pragma unroll
            for (int q = 0; q < MAXC; ++q) {
                if (q * SB < kprev) {
#pragma unroll
                    for (int p = 0; p < NR; ++p) {
                        const int e = tid + TT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                        regs[q][p] = (r < w) ? *reinterpret_cast<const uint4*>(Lrow + q * SB + (int64_t)r * ld + c * X::EPC)
                                             : make_uint4(0, 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (q * SB < kprev) {                      // uniform
                if (q) __syncthreads();                // the previous chunk has been consumed
                if (tile_wave) {
#pragma unroll
                    for (int p = 0; p < NR; ++p) {
                        const int e = tid + TT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                        *reinterpret_cast<uint4*>(chunk + r * TL::LROW + c * 16) = regs[q][p];
                    }
                }
                __syncthreads();
                if (tile_wave) mma_chunk32<T, false>(pacc, chunk, chunk, br, ch, lane);
            }
        }
    }
    acc_t acc[2];
    acc[0] = acc_zero<T>();
    acc[1] = acc_zero<T>();
    if (tile_wave) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                T v = (row == col) ? (T)1 : (T)0;                   // identity padding; strict upper part is zero
                if (row < w && col <= row) v = dval[c][r] - pacc[c][r];
                acc[c][r] = v;
            }
    }
    diag_tail<T>(acc, reinterpret_cast<T*>(pcol_), reinterpret_cast<T*>(hs_), reinterpret_cast<T*>(cs_),
                 reinterpret_cast<T*>(rall_), D, ld, w, inv, info, col_base);
}

// ---------------------------------------------------------------------------
// Panel solve for one 64-column sub-block, left-looking inside the panel, in place:
//   T = P_s - Pprev Lrow^T        Pprev = this row's kprev earlier panel columns (final),
//                                 Lrow  = the diagonal block's rows, same columns
//   X = T invL^T                  invL = 64x64 inverse of the diagonal block (lower)
// One workgroup = 32 rows (each wave 16 rows x 32 columns = 2 MFMA tiles); a
// row is read completely before it is overwritten and no other workgroup
// touches it.  Two row sets share one launch (matrix rows below the block and
// the extra right-hand-side rows of a row-wise solve).
// ---------------------------------------------------------------------------
constexpr int TR = 32;   // rows per workgroup of the panel solve
template <typename T> struct TrsmLds { static constexpr int BYTES = (2 * TR + SB) * Tile64<T>::LROW; };

template <typename T>
static __device__ __forceinline__ void trsm64_body(unsigned char* smem, T* __restrict__ Prow, int64_t ldp, int mrows, int kw, int kprev,
                                                    const T* __restrict__ Lrow, int64_t ldl,
                                                    const T* __restrict__ invL)
{
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    // smem: 32 + 32 + 64 rows = TRSM_LDS bytes: 67.6 KB (f64) -- fits next to one resident trailing-update workgroup
    unsigned char* ps = smem;                          // P_s, then T          (32 rows)
    unsigned char* as = smem + TR * TL::LROW;          // chunk of Pprev       (32 rows)
    unsigned char* bs = smem + 2 * TR * TL::LROW;      // chunk of Lrow, finally invL (64 rows)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = wave & 1, ch = wave >> 1;
    CHAIN_SETPRIO();               // panel chain: ahead of co-resident update waves
    const T* Pprev = Prow - kprev;               // the panel's earlier columns of the same rows

    v4u ra[TR * TL::CPR / 256], rb[SB * TL::CPR / 256];
    // the inverted diagonal block is needed last but depends on nothing: requested first, parked in
    // registers, so that its round trip hides behind the whole K loop instead of following it
    v4u rinv[SB * TL::CPR / 256];
#pragma unroll
    for (int p = 0; p < SB * TL::CPR / 256; ++p) {
        const int e = tid + 256 * p, r = e / TL::CPR, c = e - r * TL::CPR;
        rinv[p] = *reinterpret_cast<const v4u*>(invL + r * SB + c * X::EPC);
    }
    if (kprev > 0) {
        gload_tile64<T, TR>(ra, Pprev, ldp, mrows, SB);
        gload_tile64<T, SB>(rb, Lrow, ldl, kw, SB);
    }
    load_tile64<T, TR>(ps, Prow, ldp, mrows, kw);
    acc_t acc[2];
    acc[0] = acc_zero<T>(); acc[1] = acc_zero<T>();
    for (int kc = 0; kc < kprev; kc += SB) {
        __syncthreads();                          // previous chunk's fragments have been read
        swrite_tile64<T, TR>(as, ra);
        swrite_tile64<T, SB>(bs, rb);
        __syncthreads();
        if (kc + SB < kprev) {                    // next chunk in flight during the MFMAs
            gload_tile64<T, TR>(ra, Pprev + kc + SB, ldp, mrows, SB);
            gload_tile64<T, SB>(rb, Lrow + kc + SB, ldl, kw, SB);
        }
        mma_chunk32<T, false>(acc, as, bs, rt, ch, lane);
    }
    __syncthreads();
    // T = P_s - acc (each lane owns its accumulator elements), and stage invL
    if (kprev > 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + (lane & 15);
                T* t = reinterpret_cast<T*>(ps + row * TL::LROW) + col;
                *t -= acc[c][r];
            }
    }
    swrite_tile64<T, SB>(bs, rinv);
    __syncthreads();
    acc[0] = acc_zero<T>(); acc[1] = acc_zero<T>();
    mma_chunk32<T, true>(acc, ps, bs, rt, ch, lane);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int gc = (2 * ch + c) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = rt * 16 + X::crow(lane, r);
            if (lr < mrows && gc < kw) Prow[(int64_t)lr * ldp + gc] = acc[c][r];
        }
    }
}

// The same solve for G consecutive 32-row tiles in ONE workgroup (batched launches, round 3).  In a batch of
// many blocks the panel solves are not latency- but L2-bandwidth-bound: every 32-row workgroup streams the
// block's 64 x kprev strip of L and its 64 x 64 inverse (80-130 KB) for 16-48 KB of its own rows -- 600 MB per
// launch for 128 blocks of 2048.  Here a chunk of L is staged once per G tiles and the inverse once per
// workgroup; the tiles' operand strips follow one another through the same LDS area.
constexpr int TRSM_GROUP = 4;
template <typename T, int G>
static __device__ __forceinline__ void trsm64_group(unsigned char* smem, T* __restrict__ Prow, int64_t ldp, int mrows, int kw, int kprev,
                                                     const T* __restrict__ Lrow, int64_t ldl, const T* __restrict__ invL)
{
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    unsigned char* ps = smem;                          // P_s of one tile, then T
    unsigned char* as = smem + TR * TL::LROW;          // chunk of one tile's earlier panel columns
    unsigned char* bs = smem + 2 * TR * TL::LROW;      // chunk of Lrow, finally invL
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = wave & 1, ch = wave >> 1;
    CHAIN_SETPRIO();
    const T* Pprev = Prow - kprev;
    v4u ra[TR * TL::CPR / 256], rb[SB * TL::CPR / 256], rinv[SB * TL::CPR / 256];
#pragma unroll
    for (int p = 0; p < SB * TL::CPR / 256; ++p) {
        const int e = tid + 256 * p, r = e / TL::CPR, c = e - r * TL::CPR;
        rinv[p] = *reinterpret_cast<const v4u*>(invL + r * SB + c * X::EPC);
    }
    acc_t acc[G][2];
#pragma unroll
    for (int g = 0; g < G; ++g) { acc[g][0] = acc_zero<T>(); acc[g][1] = acc_zero<T>(); }
    if (kprev > 0) {
        gload_tile64<T, SB>(rb, Lrow, ldl, kw, SB);
        gload_tile64<T, TR>(ra, Pprev, ldp, mrows, SB);
    }
    for (int kc = 0; kc < kprev; kc += SB) {
        __syncthreads();                               // the previous chunk's fragments have been read
        swrite_tile64<T, SB>(bs, rb);
        if (kc + SB < kprev) gload_tile64<T, SB>(rb, Lrow + kc + SB, ldl, kw, SB);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g) __syncthreads();                    // the previous tile's fragments have been read
            swrite_tile64<T, TR>(as, ra);
            __syncthreads();
            // next operand strip in flight during the multiplies: the next tile's, or tile 0's of the next chunk
            if (g + 1 < G) gload_tile64<T, TR>(ra, Pprev + (int64_t)(g + 1) * TR * ldp + kc, ldp, mrows - (g + 1) * TR, SB);
            else if (kc + SB < kprev) gload_tile64<T, TR>(ra, Pprev + kc + SB, ldp, mrows, SB);
            mma_chunk32<T, false>(acc[g], as, bs, rt, ch, lane);
        }
    }
    __syncthreads();
    swrite_tile64<T, SB>(bs, rinv);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int rows_g = mrows - g * TR;             // workgroup-uniform
        if (rows_g > 0) {
            T* Pg = Prow + (int64_t)g * TR * ldp;
            __syncthreads();                           // the previous tile's T has been read; invL is in place
            load_tile64<T, TR>(ps, Pg, ldp, rows_g < TR ? rows_g : TR, kw);
            __syncthreads();
            if (kprev > 0) {
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = rt * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + (lane & 15);
                        T* t = reinterpret_cast<T*>(ps + row * TL::LROW) + col;
                        *t -= acc[g][c][r];
                    }
            }
            __syncthreads();
            acc_t x[2];
            x[0] = acc_zero<T>(); x[1] = acc_zero<T>();
            mma_chunk32<T, true>(x, ps, bs, rt, ch, lane);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int gc = (2 * ch + c) * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = rt * 16 + X::crow(lane, r);
                    if (lr < rows_g && gc < kw) Pg[(int64_t)lr * ldp + gc] = x[c][r];
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 2)
void k_trsm64(T* __restrict__ P1, int64_t ld1, int M1, int nb1,
              T* __restrict__ P2, int64_t ld2, int M2,
              int kw, int kprev, const T* __restrict__ Lrow, int64_t ldl, const T* __restrict__ invL,
              int64_t sk, int64_t sws, int64_t sb, int nchain, Riders<T> rd, int trg)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[ChainLds<T>::BYTES];
    if ((int)blockIdx.x >= nchain) {                 // riders
        run_rider<T>(smem, rd, (int)blockIdx.x - nchain, sk, sb);
        return;
    }
    P1 += (int64_t)blockIdx.y * sk;                  // batch: see k_diag64
    if (P2) P2 += (int64_t)blockIdx.y * sb;
    Lrow += (int64_t)blockIdx.y * sk;
    invL += (int64_t)blockIdx.y * sws;
    const bool second = (int)blockIdx.x >= nb1;
    T* P = second ? P2 : P1;
    const int64_t ldp = second ? ld2 : ld1;
    const int M = second ? M2 : M1;
    // trg = rows per workgroup: TR, or TR x TRSM_GROUP in batched launches (nb1 counts workgroups of that size)
    const int row0 = (second ? (int)blockIdx.x - nb1 : (int)blockIdx.x) * trg;
    if (trg == TR) trsm64_body<T>(smem, P + (int64_t)row0 * ldp, ldp, min(TR, M - row0), kw, kprev, Lrow, ldl, invL);
    else           trsm64_group<T, TRSM_GROUP>(smem, P + (int64_t)row0 * ldp, ldp, min(trg, M - row0), kw, kprev, Lrow, ldl, invL);
}

// ---------------------------------------------------------------------------
// One link of the panel chain in ONE launch (round 2).  Sub-block s of the panel has been factored
// (its inverse is in the workspace); this launch does
//   workgroups 1..   the panel solve of sub-block s for the rows BELOW the next diagonal block
//                    (and the carried rows): 32-row workgroups, exactly k_trsm64's body;
//   workgroup 0      the next diagonal block: its 64 rows' panel solve
//                    X = (P_s - Pprev Lrow^T) inv(L_ss)^T, the Schur complement
//                    S = A - [Pprev X][Pprev X]^T of the diagonal block -- every operand chunk serves
//                    both products from one LDS tile -- and the factorisation of S (diag_tail).
// The tall solve, which nothing on the chain waits for, runs in the shadow of workgroup 0's pivot
// loop, and the next diagonal block never waits for a launch of its own: per link
// max(solve, X + S + pivots) instead of diag + solve.  Operand tiles and the factorisation's LDS
// areas overlay each other (67.6 KB in all, as the panel solve alone).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(DG_NT)
void k_link(T* __restrict__ A, int64_t ld, int n, int c0, int k0, int wn,
            T* __restrict__ P2, int64_t ld2, int M2, T* __restrict__ ws, int32_t* info,
            int64_t sk, int64_t sws, int64_t sb, int nchain, Riders<T> rd)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[ChainLds<T>::BYTES];
    if ((int)blockIdx.x >= nchain) {                 // riders
        if (threadIdx.x >= 256) return;
        run_rider<T>(smem, rd, (int)blockIdx.x - nchain, sk, sb);
        return;
    }
    A += (int64_t)blockIdx.y * sk;                   // batch: see k_diag64
    ws += (int64_t)blockIdx.y * sws;
    if (P2) P2 += (int64_t)blockIdx.y * sb;
    info += blockIdx.y;
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    const int kprev = c0 - k0;
    const T* invL = ws + (int64_t)(c0 / SB) * (SB * SB);
    const T* Lrow = A + (int64_t)c0 * ld + k0;       // rows of the factored diagonal block, earlier panel columns
    const int r0 = c0 + SB;                          // first row (and column) of the next diagonal block
    if (blockIdx.x != 0) {
        // the solve uses four waves; the other five leave as whole waves (s_barrier counts the waves that
        // have not terminated, so the body's barriers are among the remaining four)
        if (threadIdx.x >= 256) return;
        const int pc = r0 + wn;
        const int M1 = n - pc, nb1 = (M1 + TR - 1) / TR;
        const int b = (int)blockIdx.x - 1;
        const bool second = b >= nb1;
        T* P = second ? P2 : A + (int64_t)pc * ld + c0;
        const int64_t ldp = second ? ld2 : ld;
        const int M = second ? M2 : M1;
        const int row0 = (second ? b - nb1 : b) * TR;
        trsm64_body<T>(smem, P + (int64_t)row0 * ldp, ldp, min(TR, M - row0), SB, kprev, Lrow, ld, invL);
        return;
    }
    constexpr int TT = 64 * DG_TW;                   // threads of the tile waves
    constexpr int NR = SB * TL::CPR / TT;            // 16-byte pieces per thread and 64 x 64 tile
    static_assert(SB * TL::LROW >= DiagLds<T>::CS, "pivot columns overlay the second operand tile");
    static_assert(SB * TL::LROW >= 2 * DiagLds<T>::PCOL + DiagLds<T>::RALL, "gather buffers overlay the first operand tile");
    unsigned char* bufA = smem;                      // own rows' chunk (both operands of S, left operand of T), then T, then X
    unsigned char* bufB = smem + SB * TL::LROW;      // Lrow chunk, then inv(L_ss)
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool tile_wave = g < DG_TW;
    const int br = (g >> 1) & 3, ch = g & 1;
    const int fcol = lane & 15;
    CHAIN_SETPRIO();
    T* Arow = A + (int64_t)r0 * ld;                  // the next diagonal block's rows
    T* D = Arow + r0;

    // everything that depends on nothing is requested first: the diagonal block and P_s in
    // accumulator layout, inv(L_ss) and the first operand chunks in staging registers
    T dval[2][4], pval[2][4];
    v4u rI[NR], rA[NR], rB[NR];
    if (tile_wave) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                dval[c][r] = (row < wn && col <= row) ? D[(int64_t)row * ld + col] : (T)0;
                pval[c][r] = (row < wn) ? Arow[(int64_t)row * ld + c0 + col] : (T)0;
            }
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = tid + TT * p, r = e / TL::CPR, c = e - r * TL::CPR;
            rI[p] = *reinterpret_cast<const v4u*>(invL + r * SB + c * X::EPC);
            if (kprev > 0) {
                rA[p] = (r < wn) ? *reinterpret_cast<const v4u*>(Arow + k0 + (int64_t)r * ld + c * X::EPC) : v4u_zero();
                rB[p] = *reinterpret_cast<const v4u*>(Lrow + (int64_t)r * ld + c * X::EPC);
            }
        }
    }
    acc_t accT[2], accS[2];
    accT[0] = acc_zero<T>(); accT[1] = acc_zero<T>();
    accS[0] = acc_zero<T>(); accS[1] = acc_zero<T>();
    for (int kc = 0; kc < kprev; kc += SB) {
        if (kc) __syncthreads();                     // the previous chunk has been consumed
        if (tile_wave) {
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const int e = tid + TT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                *reinterpret_cast<v4u*>(bufA + r * TL::LROW + c * 16) = rA[p];
                *reinterpret_cast<v4u*>(bufB + r * TL::LROW + c * 16) = rB[p];
            }
        }
        __syncthreads();
        if (tile_wave) {
            if (kc + SB < kprev) {                   // next chunk in flight during the multiplies
#pragma unroll
                for (int p = 0; p < NR; ++p) {
                    const int e = tid + TT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                    rA[p] = (r < wn) ? *reinterpret_cast<const v4u*>(Arow + k0 + kc + SB + (int64_t)r * ld + c * X::EPC)
                                     : v4u_zero();
                    rB[p] = *reinterpret_cast<const v4u*>(Lrow + kc + SB + (int64_t)r * ld + c * X::EPC);
                }
            }
            mma_chunk32<T, false>(accT, bufA, bufB, br, ch, lane);
            mma_chunk32<T, false>(accS, bufA, bufA, br, ch, lane);
        }
    }
    if (kprev > 0) __syncthreads();
    // T = P_s - accT (each lane owns its accumulator elements) as the left operand, inv(L_ss) as the right one
    if (tile_wave) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                *(reinterpret_cast<T*>(bufA + row * TL::LROW) + col) = pval[c][r] - accT[c][r];
            }
        swrite_tile64<T, SB, TT>(bufB, rI);
    }
    lds_barrier();
    acc_t accX[2];
    accX[0] = acc_zero<T>(); accX[1] = acc_zero<T>();
    if (tile_wave) {
        mma_chunk32<T, true>(accX, bufA, bufB, br, ch, lane);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                if (row < wn) Arow[(int64_t)row * ld + c0 + col] = accX[c][r];
            }
    }
    lds_barrier();                                   // T and inv(L_ss) have been read
    if (tile_wave) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                *(reinterpret_cast<T*>(bufA + row * TL::LROW) + col) = accX[c][r];     // rows >= wn are zero
            }
    }
    lds_barrier();
    acc_t acc[2];
    acc[0] = acc_zero<T>();
    acc[1] = acc_zero<T>();
    if (tile_wave) {
        mma_chunk32<T, false>(accS, bufA, bufA, br, ch, lane);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = br * 16 + X::crow(lane, r), col = (2 * ch + c) * 16 + fcol;
                T v = (row == col) ? (T)1 : (T)0;                   // identity padding; strict upper part is zero
                if (row < wn && col <= row) v = dval[c][r] - accS[c][r];
                acc[c][r] = v;
            }
    }
    // The second tile is dead since the barrier above: S goes there (diag_tail) and becomes the pivot columns;
    // the first is read by the last multiply until diag_tail's barrier and then holds the gather buffers.
    T* pcol = reinterpret_cast<T*>(bufA);
    T* hs   = reinterpret_cast<T*>(bufA + DiagLds<T>::PCOL);
    T* rall = reinterpret_cast<T*>(bufA + 2 * DiagLds<T>::PCOL);
    diag_tail<T>(acc, pcol, hs, reinterpret_cast<T*>(bufB), rall, D, ld, wn,
                 ws + (int64_t)(r0 / SB) * (SB * SB), info, r0);
}

// ---------------------------------------------------------------------------
// Four-wave forms of the diagonal factorisation and of the link (round 2).  A nine-wave workgroup
// needs a compute unit that BOTH resident trailing-update workgroups have left (three of its waves
// share one SIMD's registers), so beside a running update it waits for the update's last generation;
// a four-wave workgroup (one wave per SIMD, <= 256 registers) fits beside ONE update workgroup and
// is dispatched, by queue priority, as soon as any update workgroup retires.
//   waves 0..2   tile waves: the sixteen 16x16 tiles of the combined array dealt round-robin
//                (tile t = 4 row-tile + column-tile belongs to wave t mod 3: 6 / 5 / 5 tiles);
//   wave 3       the pivot wave, alone on its SIMD.
// The left-looking products before the factorisation use all four waves in row-tile layout
// (wave w = rows 16 w ..: mma_chunk64) and hand the Schur complement over through LDS (`cs`, whose
// first use inside the loop is the pivot wave's write of block 0 after the first barrier).
// ---------------------------------------------------------------------------
constexpr int Q_TW = 3;               // tile waves
constexpr int Q_NT = 256;             // threads

// Schur complement from row-tile accumulators to `cs` (identity padding beyond w, zeros above the diagonal)
template <typename T>
static __device__ __forceinline__ void schur_to_lds(T* __restrict__ cs, const T (&dval)[4][4],
                                                     const typename Mx<T>::acc_t (&sub)[4], int wave, int lane, int w)
{
    using X = Mx<T>;
    constexpr int LS = SB + 2;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            T v = (row == col) ? (T)1 : (T)0;
            if (row < w && col <= row) v = dval[c][r] - sub[c][r];
            cs[row * LS + col] = v;
        }
    // the other waves read these words right behind the caller's barrier: read the last one back first (lds_settle)
    lds_settle(&cs[(wave * 16 + X::crow(lane, 3)) * LS + 3 * 16 + (lane & 15)]);
}

template <typename T>
__global__ __launch_bounds__(Q_NT, 2)
void k_diag64q(T* __restrict__ D, int64_t ld, int w, const T* __restrict__ Lrow, int kprev,
               T* __restrict__ inv, int32_t* info, int col_base, int64_t sk, int64_t sws, int64_t sb, Riders<T> rd)
{
    __shared__ __attribute__((aligned(16))) unsigned char chunk[RIDER_LDS];           // Lrow chunk / a rider's tiles
    if (blockIdx.x != 0) {                           // riders
        run_rider<T>(chunk, rd, (int)blockIdx.x - 1, sk, sb);
        return;
    }
    D += (int64_t)blockIdx.y * sk;
    Lrow += (int64_t)blockIdx.y * sk;
    inv += (int64_t)blockIdx.y * sws;
    info += blockIdx.y;
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    __shared__ __attribute__((aligned(16))) unsigned char pcol_[DiagLds<T>::PCOL];
    __shared__ __attribute__((aligned(16))) unsigned char hs_[DiagLds<T>::PCOL];
    __shared__ __attribute__((aligned(16))) unsigned char cs_[DiagLds<T>::CS];
    __shared__ __attribute__((aligned(16))) unsigned char rall_[DiagLds<T>::RALL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    CHAIN_SETPRIO();
    T dval[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            dval[c][r] = (row < w && col <= row) ? D[(int64_t)row * ld + col] : (T)0;
        }
    acc_t pacc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) pacc[c] = acc_zero<T>();
    if (kprev > 0) {
        // all (up to four: kprev = 256 when the block takes its head update here) chunks of Lrow are
        // requested at once: ONE exposed round trip -- beside a running trailing update a dependent global
        // round trip costs several microseconds, not one
        constexpr int NR = SB * TL::CPR / Q_NT;
        constexpr int MAXC = CIMRGP_NB / SB;
        v4u regs[MAXC][NR];
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (q * SB < kprev) {
#pragma unroll
                for (int p = 0; p < NR; ++p) {
                    const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                    regs[q][p] = (r < w) ? *reinterpret_cast<const v4u*>(Lrow + q * SB + (int64_t)r * ld + c * X::EPC) : v4u_zero();
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MAXC; ++q) {
            if (q * SB < kprev) {                      // uniform
                if (q) __syncthreads();                // the previous chunk has been consumed
#pragma unroll
                for (int p = 0; p < NR; ++p) {
                    const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
                    *reinterpret_cast<v4u*>(chunk + r * TL::LROW + c * 16) = regs[q][p];
                }
                __syncthreads();
                mma_chunk64<T, false>(pacc, chunk, chunk, wave, lane);
            }
        }
    }
    schur_to_lds<T>(reinterpret_cast<T*>(cs_), dval, pacc, wave, lane, w);
    __syncthreads();
    diag_tail_lds<T, Q_TW, Q_NT>(wave < Q_TW ? wave : -1, wave == Q_TW, reinterpret_cast<T*>(pcol_), reinterpret_cast<T*>(hs_),
                                 reinterpret_cast<T*>(cs_), reinterpret_cast<T*>(rall_), D, ld, w, inv, info, col_base);
}

// k_link with four-wave workgroups throughout (see k_link for what a link does).
template <typename T>
__global__ __launch_bounds__(Q_NT, 2)
void k_linkq(T* __restrict__ A, int64_t ld, int n, int c0, int k0, int wn,
             T* __restrict__ P2, int64_t ld2, int M2, T* __restrict__ ws, int32_t* info,
             int64_t sk, int64_t sws, int64_t sb, int nchain, Riders<T> rd, int trg)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[ChainLds<T>::BYTES];
    if ((int)blockIdx.x >= nchain) {                 // riders
        run_rider<T>(smem, rd, (int)blockIdx.x - nchain, sk, sb);
        return;
    }
    A += (int64_t)blockIdx.y * sk;
    ws += (int64_t)blockIdx.y * sws;
    if (P2) P2 += (int64_t)blockIdx.y * sb;
    info += blockIdx.y;
    using X = Mx<T>;
    using TL = Tile64<T>;
    using acc_t = typename X::acc_t;
    const int kprev = c0 - k0;
    const T* invL = ws + (int64_t)(c0 / SB) * (SB * SB);
    const T* Lrow = A + (int64_t)c0 * ld + k0;
    const int r0 = c0 + SB;
    if (blockIdx.x != 0) {
        // trg = rows per solve workgroup: TR, or TR x TRSM_GROUP in batched launches (k_trsm64)
        const int pc = r0 + wn;
        const int M1 = n - pc, nb1 = (M1 + trg - 1) / trg;
        const int b = (int)blockIdx.x - 1;
        const bool second = b >= nb1;
        T* P = second ? P2 : A + (int64_t)pc * ld + c0;
        const int64_t ldp = second ? ld2 : ld;
        const int M = second ? M2 : M1;
        const int row0 = (second ? b - nb1 : b) * trg;
        if (trg == TR) trsm64_body<T>(smem, P + (int64_t)row0 * ldp, ldp, min(TR, M - row0), SB, kprev, Lrow, ld, invL);
        else           trsm64_group<T, TRSM_GROUP>(smem, P + (int64_t)row0 * ldp, ldp, min(trg, M - row0), SB, kprev, Lrow, ld, invL);
        return;
    }
    constexpr int NR = SB * TL::CPR / Q_NT;
    static_assert(SB * TL::LROW >= DiagLds<T>::CS, "pivot columns overlay the second operand tile");
    static_assert(SB * TL::LROW >= 2 * DiagLds<T>::PCOL + DiagLds<T>::RALL, "gather buffers overlay the first operand tile");
    unsigned char* bufA = smem;
    unsigned char* bufB = smem + SB * TL::LROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    CHAIN_SETPRIO();
    T* Arow = A + (int64_t)r0 * ld;
    T* D = Arow + r0;

    T pval[4][4];
    v4u rI[NR], rA[NR], rB[NR];
    // inv(L_ss) is requested when the staging registers of the last operand chunk fall free (the
    // kernel is held to 256 registers so that a workgroup fits beside a trailing-update workgroup)
    auto fetch_inv = [&]() {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
            rI[p] = *reinterpret_cast<const v4u*>(invL + r * SB + c * X::EPC);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
                pval[c][r] = (row < wn) ? Arow[(int64_t)row * ld + c0 + col] : (T)0;
            }
    };
    if (kprev > 0) {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
            rA[p] = (r < wn) ? *reinterpret_cast<const v4u*>(Arow + k0 + (int64_t)r * ld + c * X::EPC) : v4u_zero();
            rB[p] = *reinterpret_cast<const v4u*>(Lrow + (int64_t)r * ld + c * X::EPC);
        }
    } else {
        fetch_inv();
    }
    acc_t accT[4], accS[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { accT[c] = acc_zero<T>(); accS[c] = acc_zero<T>(); }
    auto stage = [&]() {                             // staging registers -> operand tiles
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
            *reinterpret_cast<v4u*>(bufA + r * TL::LROW + c * 16) = rA[p];
            *reinterpret_cast<v4u*>(bufB + r * TL::LROW + c * 16) = rB[p];
        }
    };
    // all chunks but the last: the next chunk in flight during the multiplies
    for (int kc = 0; kc + SB < kprev; kc += SB) {
        if (kc) __syncthreads();
        stage();
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
            rA[p] = (r < wn) ? *reinterpret_cast<const v4u*>(Arow + k0 + kc + SB + (int64_t)r * ld + c * X::EPC) : v4u_zero();
            rB[p] = *reinterpret_cast<const v4u*>(Lrow + kc + SB + (int64_t)r * ld + c * X::EPC);
        }
        mma_chunk64<T, false>(accT, bufA, bufB, wave, lane);
        mma_chunk64<T, false>(accS, bufA, bufA, wave, lane);
    }
    // the last chunk: inv(L_ss) and P_s in flight instead (the staging registers are free by then)
    if (kprev > 0) {
        if (kprev > SB) __syncthreads();
        stage();
        __syncthreads();
        fetch_inv();
        mma_chunk64<T, false>(accT, bufA, bufB, wave, lane);
        mma_chunk64<T, false>(accS, bufA, bufA, wave, lane);
    }
    if (kprev > 0) __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            *(reinterpret_cast<T*>(bufA + row * TL::LROW) + col) = pval[c][r] - accT[c][r];
        }
#pragma unroll
    for (int p = 0; p < NR; ++p) {
        const int e = tid + Q_NT * p, r = e / TL::CPR, c = e - r * TL::CPR;
        *reinterpret_cast<v4u*>(bufB + r * TL::LROW + c * 16) = rI[p];
    }
    // the diagonal block itself: needed last, requested now that the staging registers are free
    T dval[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            dval[c][r] = (row < wn && col <= row) ? D[(int64_t)row * ld + col] : (T)0;
        }
    lds_barrier();
    acc_t accX[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) accX[c] = acc_zero<T>();
    mma_chunk64<T, true>(accX, bufA, bufB, wave, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            if (row < wn) Arow[(int64_t)row * ld + c0 + col] = accX[c][r];
        }
    lds_barrier();                                   // T and inv(L_ss) have been read
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + X::crow(lane, r), col = c * 16 + (lane & 15);
            *(reinterpret_cast<T*>(bufA + row * TL::LROW) + col) = accX[c][r];
        }
    lds_barrier();
    mma_chunk64<T, false>(accS, bufA, bufA, wave, lane);
    // S into the second tile (dead since the barrier above), which becomes `cs`; the first tile is
    // read by the multiply above until the barrier below and then holds the gather buffers
    schur_to_lds<T>(reinterpret_cast<T*>(bufB), dval, accS, wave, lane, wn);
    lds_barrier();
    T* pcol = reinterpret_cast<T*>(bufA);
    T* hs   = reinterpret_cast<T*>(bufA + DiagLds<T>::PCOL);
    T* rall = reinterpret_cast<T*>(bufA + 2 * DiagLds<T>::PCOL);
    diag_tail_lds<T, Q_TW, Q_NT>(wave < Q_TW ? wave : -1, wave == Q_TW, pcol, hs, reinterpret_cast<T*>(bufB), rall, D, ld, wn,
                                 ws + (int64_t)(r0 / SB) * (SB * SB), info, r0);
}

}  // namespace
}  // namespace cimrgp
