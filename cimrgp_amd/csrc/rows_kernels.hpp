// Device code of the Cholesky factorisation beside the panel chain: the 256-wide solve of carried rows
// (k_trsm256, k_rows_step), the 256 x 256 inverses of the diagonal blocks (k_invT_panel) and the gate that holds
// the chain until a combined update has stored its head tiles (k_gate).  Included by potrf.hip only, after
// chain_kernels.hpp: the whole factorisation stays one translation unit.
#pragma once
#include "chain_kernels.hpp"

namespace cimrgp {
namespace {

// All four sub-steps of a panel for rows that take no part in the factorisation itself (the
// right-hand-side rows of a row-wise solve): one launch per panel instead of four.  A row
// block only ever reads its own earlier results, written by this same workgroup.
template <typename T>
__global__ __launch_bounds__(256)
void k_trsm256(T* __restrict__ P, int64_t ldp, int M, int w, const T* __restrict__ Lpanel, int64_t ldl,
               const T* __restrict__ inv64, int64_t sp = 0, int64_t sk = 0, int64_t sws = 0)
{
    P += (int64_t)blockIdx.y * sp;                   // batch: see k_diag64
    Lpanel += (int64_t)blockIdx.y * sk;
    inv64 += (int64_t)blockIdx.y * sws;
    const int row0 = (int)blockIdx.x * TR;
    const int mrows = min(TR, M - row0);
    __shared__ __attribute__((aligned(16))) unsigned char smem[TrsmLds<T>::BYTES];
    for (int c0 = 0; c0 < w; c0 += SB) {
        if (c0) __syncthreads();                 // this workgroup's stores of the previous sub-step are visible
        trsm64_body<T>(smem, P + (int64_t)row0 * ldp + c0, ldp, mrows, min(SB, w - c0), c0,
                       Lpanel + (int64_t)c0 * ldl, ldl, inv64 + (int64_t)(c0 / SB) * (SB * SB));
    }
}

// ---------------------------------------------------------------------------
// Round 4: ONE launch per panel for the carried rows' own chain.  Panel p of the rows needs
//     W_p = (B_p - W_{p-1} L[p, p-1]^T) L_pp^-T
// -- the update by the previous panel (everything older has been applied by the bulk "far" updates, which are
// off this chain) and the 256-wide solve.  Until round 4 these were two launches of general kernels (a 64-tile
// update of 132 workgroups, 38-65 us, then k_trsm256, 34-55 us: both latency-bound) and the rows fell eleven
// panels behind a factorisation whose own chain takes 93-125 us per panel.  Here a workgroup owns 16 rows (one
// MFMA row tile) for both parts:
//   * wave w owns the four 16-column tiles  64 j + 16 w  (j = 0..3: one of every 64-column sub-block), so that in
//     sub-step j all four waves work on sub-block j and each already holds its share of it;
//   * the right operand (rows of L / of the 64 x 64 inverses) goes from global memory STRAIGHT into the
//     matrix-core operand registers -- lane (n, q) takes 32 contiguous bytes of row n per 128-byte chunk of K
//     (the k order inside a chunk is a permutation, the same one on both operands), so a wave's request is 16
//     rows x 128 bytes, whole cache lines, and nobody waits at a barrier for a staging buffer; the loads run a
//     ring of chunks ahead of the multiplies, through the barriers (LDS-scoped fences: a __syncthreads() would
//     drain them);
//   * the left operands (W_{p-1}'s rows, the solved sub-blocks, the 16 x 64 sub-block being solved) live in LDS.
// Sub-step j: T_j = B_j - W_{p-1} L[j, p-1]^T (phase 1, all j at once) - sum_{i<j} W_i L[j, i]^T, then
// W_j = T_j inv_j^T through LDS (two barriers per sub-step).  Full panels only (w = 256, previous panel 256 or
// none); ragged last panels keep the two-launch form.
// ---------------------------------------------------------------------------
template <typename T> struct RowsStep {
    static constexpr int R = 16;                                   // rows per workgroup
    static constexpr int CHE = 128 / (int)sizeof(T);               // elements per 128-byte chunk of K
    static constexpr int NCP = CIMRGP_NB / CHE;                    // chunks of the previous panel: 16 (f64) / 8 (f32)
    static constexpr int NCS = SB / CHE;                           // chunks of a 64-column sub-block: 4 / 2
    static constexpr int LPE = 32 / (int)sizeof(T);                // elements a lane takes per chunk (32 bytes)
    static constexpr int ASTR = CIMRGP_NB * (int)sizeof(T) + 16;   // LDS row strides: 16 bytes of padding
    static constexpr int TSTR = SB * (int)sizeof(T) + 16;
    static constexpr int BYTES = 2 * R * ASTR + R * TSTR;
    static constexpr int RING1 = 3;                                // phase 1: chunks in flight (4 tiles each)
    static constexpr int RING2 = 8;                                // phase 2: chunks in flight (1 tile each)
    static constexpr int P2_TOTAL = NCS * (1 + 2 + 3 + 4);
};

template <typename T, bool HAS_PREV>
__global__ __launch_bounds__(256)
void k_rows_step(T* __restrict__ P, int64_t ldp, int M, const T* __restrict__ Lrow, int64_t ldl, const T* __restrict__ inv64,
                 const T* __restrict__ Pprev = nullptr, int64_t ldprev = 0, int b_zero = 0, int ny = 1,
                 int64_t sp = 0, int64_t sl = 0, int64_t sws = 0, int64_t sprev = 0,
                 int64_t sp2 = 0, int64_t sl2 = 0, int64_t sws2 = 0)
{
    // Pprev: the previous panel's solved rows live elsewhere (row r of this launch at Pprev + r * ldprev) instead of in
    // the 256 columns left of P; b_zero: B_p = 0 (1) or the identity (2), not read.  blockIdx.y = i + ny * j: problem i of ny with strides
    // (sp, sl, sws, sprev), inside matrix j of a batch with strides (sp2, sl2, sws2; Pprev moves with sp2).  These
    // serve the 512-wide inverses of the skinny backward solve (build_invT).
    {
        const int yi = (int)blockIdx.y % ny, yj = (int)blockIdx.y / ny;
        P += (int64_t)yi * sp + (int64_t)yj * sp2;
        Lrow += (int64_t)yi * sl + (int64_t)yj * sl2;
        inv64 += (int64_t)yi * sws + (int64_t)yj * sws2;
        if (Pprev) Pprev += (int64_t)yi * sprev + (int64_t)yj * sp2;
    }
    using X = Mx<T>;
    using acc_t = typename X::acc_t;
    using RS = RowsStep<T>;
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    constexpr int KPREV = HAS_PREV ? CIMRGP_NB : 0;
    __shared__ __attribute__((aligned(16))) unsigned char smem[RS::BYTES];
    unsigned char* aprev = smem;                       // W_{p-1}: R rows x 256
    unsigned char* wcur  = smem + RS::R * RS::ASTR;    // W_p as it is solved
    unsigned char* tbuf  = smem + 2 * RS::R * RS::ASTR;   // T_j: R rows x 64
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = (int)blockIdx.x * RS::R;
    const int mrows = min(RS::R, M - row0);
    T* Prow = P + (int64_t)row0 * ldp;                 // this workgroup's rows, first column of panel p
    const int fn = lane & 15, fq = lane >> 4;
    const int ctile = 16 * wave + fn;                  // this lane's column inside a 64-column sub-block

    // W_{p-1}'s rows: requested first, written to LDS after everything else has been requested
    v4u stg[HAS_PREV ? RS::NCP / 2 : 1];
    const int sr = tid >> 4, st16 = tid & 15;
    if (HAS_PREV) {
        // rows past the end: a valid row's values, never stored
        const T* src = Pprev ? Pprev + (int64_t)(row0 + min(sr, mrows - 1)) * ldprev : Prow - KPREV + (int64_t)min(sr, mrows - 1) * ldp;
#pragma unroll
        for (int i = 0; i < RS::NCP / 2; ++i) stg[i] = *reinterpret_cast<const v4u*>(src + (i * 16 + st16) * X::EPC);
    }
    // FP32: B is kept apart and the products are accumulated from zero, B added once where T_j is formed (gemm_tile.hpp has
    // the reason: started as B, every entry took each of its products with a rounding at its own size)
    constexpr bool APART = sizeof(T) == 4;
    acc_t acc[4];
    acc_t bini[APART ? 4 : 1];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const T v = (b_zero == 0) ? Prow[(int64_t)min(X::crow(lane, r), mrows - 1) * ldp + SB * j + ctile]
                      : (b_zero == 2 && row0 + X::crow(lane, r) == SB * j + ctile) ? (T)1 : (T)0;
            if constexpr (APART) { bini[j][r] = v; acc[j][r] = (T)0; }
            else acc[j][r] = v;
        }

    // right-operand rows of this lane: rows SB j + ctile of the panel's row block of L, and of the inverses
    const T* lp[4];
    const T* ip[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lp[j] = Lrow + (int64_t)(SB * j + ctile) * ldl + fq * RS::LPE;
        ip[j] = inv64 + (int64_t)j * (SB * SB) + ctile * SB + fq * RS::LPE;
    }
    // phase 2's operand stream in the order it is consumed: sub-step j = j NCS chunks of L[j, 0 .. 64 j) (behind
    // the previous panel's 256 columns), then NCS chunks of inv_j
    auto p2_addr = [&](int p) -> const T* {
        int j = 0, base = 0;
#pragma unroll
        for (j = 0; j < 4; ++j) {
            const int len = (j + 1) * RS::NCS;
            if (p < base + len) break;
            base += len;
        }
        const int c = p - base;
        return (c < j * RS::NCS) ? lp[j] + KPREV + c * RS::CHE : ip[j] + (c - j * RS::NCS) * RS::CHE;
    };
    v4u ring2[RS::RING2][2];
#define ROWS_P2_LOAD(p_)                                                                   \
    {                                                                                      \
        const T* q_ = p2_addr(p_);                                                         \
        ring2[(p_) % RS::RING2][0] = *reinterpret_cast<const v4u*>(q_);                    \
        ring2[(p_) % RS::RING2][1] = *reinterpret_cast<const v4u*>(q_ + X::EPC);           \
    }
    // the four 8-byte k-slots of a lane's 32 bytes
#define ROWS_SLOT(v_, s_) ((s_) == 0 ? make_uint2((v_)[0].x, (v_)[0].y) : (s_) == 1 ? make_uint2((v_)[0].z, (v_)[0].w) \
                           : (s_) == 2 ? make_uint2((v_)[1].x, (v_)[1].y) : make_uint2((v_)[1].z, (v_)[1].w))

    if (HAS_PREV) {
        v4u ring1[RS::RING1][4][2];
#define ROWS_P1_LOAD(c_)                                                                   \
    {                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                    \
            const T* q_ = lp[j] + (c_) * RS::CHE;                                          \
            ring1[(c_) % RS::RING1][j][0] = *reinterpret_cast<const v4u*>(q_);             \
            ring1[(c_) % RS::RING1][j][1] = *reinterpret_cast<const v4u*>(q_ + X::EPC);    \
        }                                                                                  \
    }
#pragma unroll
        for (int c = 0; c < RS::RING1; ++c) ROWS_P1_LOAD(c)
#pragma unroll
        for (int i = 0; i < RS::NCP / 2; ++i)
            *reinterpret_cast<v4u*>(aprev + sr * RS::ASTR + (i * 16 + st16) * 16) = stg[i];
        lds_barrier();                                                   // W_{p-1}'s rows are in LDS
        const unsigned char* abase = aprev + fn * RS::ASTR + fq * 32;
#pragma unroll
        for (int c = 0; c < RS::NCP; ++c) {
            v4u a[2];
            a[0] = *reinterpret_cast<const v4u*>(abase + c * 128);
            a[1] = *reinterpret_cast<const v4u*>(abase + c * 128 + 16);
            if (c == RS::NCP - 1) {
                // the ring drains: phase 2's first chunks take its place
#pragma unroll
                for (int p = 0; p < RS::RING2; ++p) ROWS_P2_LOAD(p)
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint2 an = ROWS_SLOT(a, s);          // negated by the multiply itself (Mx<T>::mma_neg)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = X::mma_neg(an, ROWS_SLOT(ring1[c % RS::RING1][j], s), acc[j]);
            }
            if (c + RS::RING1 < RS::NCP) ROWS_P1_LOAD(c + RS::RING1)
        }
#undef ROWS_P1_LOAD
    } else {
#pragma unroll
        for (int p = 0; p < RS::RING2; ++p) ROWS_P2_LOAD(p)
    }

    int pos = 0;                                       // position in phase 2's stream (a constant once unrolled)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // T_j's share of this wave: the solved sub-blocks 0 .. j-1 of this panel against L[j, 0 .. 64 j)
        const unsigned char* wbase = wcur + fn * RS::ASTR + fq * 32;
#pragma unroll
        for (int c = 0; c < j * RS::NCS; ++c, ++pos) {
            v4u a[2];
            a[0] = *reinterpret_cast<const v4u*>(wbase + c * 128);
            a[1] = *reinterpret_cast<const v4u*>(wbase + c * 128 + 16);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[j] = X::mma_neg(ROWS_SLOT(a, s), ROWS_SLOT(ring2[pos % RS::RING2], s), acc[j]);
            if (pos + RS::RING2 < RS::P2_TOTAL) ROWS_P2_LOAD(pos + RS::RING2)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            T tj = acc[j][r];
            if constexpr (APART) tj += bini[j][r];
            *reinterpret_cast<T*>(tbuf + X::crow(lane, r) * RS::TSTR + ctile * (int)sizeof(T)) = tj;
        }
        lds_barrier();                                                   // T_j complete
        acc_t x = acc_zero<T>();
        const unsigned char* tbase = tbuf + fn * RS::TSTR + fq * 32;
#pragma unroll
        for (int c = 0; c < RS::NCS; ++c, ++pos) {
            v4u a[2];
            a[0] = *reinterpret_cast<const v4u*>(tbase + c * 128);
            a[1] = *reinterpret_cast<const v4u*>(tbase + c * 128 + 16);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                x = X::mma(ROWS_SLOT(a, s), ROWS_SLOT(ring2[pos % RS::RING2], s), x);
            if (pos + RS::RING2 < RS::P2_TOTAL) ROWS_P2_LOAD(pos + RS::RING2)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = X::crow(lane, r);
            if (j < 3) *reinterpret_cast<T*>(wcur + lr * RS::ASTR + (SB * j + ctile) * (int)sizeof(T)) = x[r];
            if (lr < mrows) Prow[(int64_t)lr * ldp + SB * j + ctile] = x[r];
        }
        if (j < 3) lds_barrier();                                        // W_j is in LDS; T's buffer is free
    }
#undef ROWS_P2_LOAD
#undef ROWS_SLOT
}

// ---------------------------------------------------------------------------
// 256x256 inverses of the diagonal blocks, for the skinny solves: the identity is
// carried through the panel solve, batched over ALL panels (blockIdx.y):
// invT_p = I L_pp^-T = (L_pp^-1)^T  (upper triangular, row r = column r of L_pp^-1),
// stored 256 x 256 row-major per panel.  (Rounds 1-2: an init pass and one launch per
// 64-column sub-step.)
// ---------------------------------------------------------------------------
// ONE launch (round 3): a 32-row strip of the 256 x 256 block depends on no other strip, so its
// workgroup runs the four 64-column sub-steps itself (its own earlier columns are read back from global memory
// behind a workgroup barrier), writes the identity it starts from instead of a separate init pass, and skips
// what is known to be zero: strip i has nothing left of column 32 i.  (Five dependent launches at the end of
// every factorisation were 53 us of a N = 8192 step; 0.94 ms of a 128 x 2048 layer.)
template <typename T>
__global__ __launch_bounds__(256)
void k_invT_panel(T* __restrict__ invT, const T* __restrict__ L, int64_t ld, int n, const T* __restrict__ inv64,
                  int64_t sk = 0, int64_t sws = 0, int p0 = 0)
{
    invT += (int64_t)blockIdx.z * sws;
    L += (int64_t)blockIdx.z * sk;
    inv64 += (int64_t)blockIdx.z * sws;
    const int p = p0 + (int)blockIdx.y, strip = blockIdx.x;
    const int k0 = p * CIMRGP_NB;
    const int w = min(CIMRGP_NB, n - k0);
    T* blk = invT + (int64_t)p * (CIMRGP_NB * CIMRGP_NB) + (int64_t)strip * TR * CIMRGP_NB;
    for (int e = threadIdx.x; e < TR * CIMRGP_NB; e += 256) {
        const int r = strip * TR + (e >> 8), c = e & 255;
        blk[e] = (r == c && r < w) ? (T)1 : (T)0;
    }
    __shared__ __attribute__((aligned(16))) unsigned char smem[TrsmLds<T>::BYTES];
    const int first = (strip * TR) / SB;                 // first 64-column block with a non-zero in this strip
    for (int s = first; s < CIMRGP_NB / SB; ++s) {
        const int c0 = k0 + SB * s;
        const int kw = min(SB, n - c0);
        if (kw <= 0) break;
        __syncthreads();                                  // the strip's earlier columns (and the identity) are stored; LDS is free
        trsm64_body<T>(smem, blk + SB * s, CIMRGP_NB, TR, kw, SB * (s - first), L + (int64_t)c0 * ld + k0 + SB * first, ld,
                       inv64 + (int64_t)(c0 / SB) * (SB * SB));
    }
}

// The panel chain's wait for the head tiles of a combined (head-first) persistent update: ONE workgroup polls the
// count of stored head tiles (k_gemm_nt_pers adds 1 per tile behind an agent-scope release) and ends; the
// chain's next launch follows it in queue order.  One resident wave cannot starve the update of compute
// units (a poll inside the wide panel-solve launch could: its hundreds of workgroups would hold the units the
// persistent workgroups are waiting for).  The poll is bounded by the constant 100 MHz clock (s_memrealtime):
// after GATE_TIMEOUT_TICKS = 2 s without the count the factorisation is flagged with CIMRGP_INFO_WATCHDOG
// (include/cimrgp.h: a SCHEDULE failure, not a numerical one) instead of hanging the device.
constexpr long long GATE_TIMEOUT_TICKS = 200000000ll;
__global__ void k_gate(const int* __restrict__ flag, int expected, int32_t* info)
{
    if (threadIdx.x == 0) {
        const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < expected) {
            __builtin_amdgcn_s_sleep(64);
            if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > GATE_TIMEOUT_TICKS) {
                atomicCAS(info, 0, CIMRGP_INFO_WATCHDOG);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
}

}  // namespace
}  // namespace cimrgp
