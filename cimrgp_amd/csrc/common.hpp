// Shared device/host helpers for the gfx950 dense-GP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <type_traits>

#include "../../include/cimrgp.h"

namespace cimrgp {

// ---------------------------------------------------------------- errors ----
void set_error(const std::string& msg);
int  fail(const char* fn, const char* what);
int  check_hip(hipError_t e, const char* fn, const char* what);

#define CIMRGP_REQUIRE(cond, fn, what) \
    do { if (!(cond)) return ::cimrgp::fail(fn, what); } while (0)
#define CIMRGP_LAUNCH_CHECK(fn) \
    do { hipError_t e__ = hipGetLastError(); \
         if (e__ != hipSuccess) return ::cimrgp::check_hip(e__, fn, "kernel launch"); } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The limits of every entry point: at most 8 input dimensions and 8 outputs (they size __shared__ and register arrays)
constexpr int MAXD = 8;
constexpr int MAXQ = 8;
// Row pitch (elements) of the matrices the library lays out itself: device.padded_ld's rule (a multiple of 16, never of 512)
static inline int64_t padded_ld(int64_t n) { const int64_t ld = (n + 15) / 16 * 16; return ld % 512 == 0 ? ld + 16 : ld; }

// ------------------------------------------------------------ MFMA traits ----
// 16x16x4 matrix-core tiles, one 8-byte "k-slot" per lane per operand:
//   lane l supplies A[row = l & 15][kslot = l >> 4] and B^T[col = l & 15][kslot = l >> 4].
// f64: a slot is one double  -> one v_mfma_f64_16x16x4_f64.
// f32: a slot is two floats  -> two v_mfma_f32_16x16x4_f32 (k order inside the
//      slot is irrelevant because A and B use the same slot->k map).
template <typename T> struct Mx;

template <> struct Mx<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static constexpr int EPC = 2;     // elements per 16-byte chunk
    static constexpr int EPS = 1;     // elements per 8-byte k-slot
    // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 r
    static __device__ __forceinline__ int crow(int lane, int r) { return (lane >> 4) + 4 * r; }
    static __device__ __forceinline__ uint2 neg(uint2 a) { a.y ^= 0x80000000u; return a; }
    static __device__ __forceinline__ acc_t mma(uint2 a, uint2 b, acc_t c) {
        double da = __hiloint2double((int)a.y, (int)a.x);
        double db = __hiloint2double((int)b.y, (int)b.x);
        return __builtin_amdgcn_mfma_f64_16x16x4f64(da, db, c, 0, 0, 0);
    }
    // c - a b: the FP64 matrix-core instruction negates an operand itself (on gfx940+ the builtin's last argument is
    // neg:[A, B, C] for v_mfma_f64_*: the assembler prints `neg:[1,0,0]`), so no vector instruction is spent on the sign
    // (round 5: the update kernels flipped the sign bit of every A fragment with a v_xor -- 16 per stage and wave, each
    // taking a vector issue slot the next multiply had to wait for).  Bit-identical: negation is exact.
    static __device__ __forceinline__ acc_t mma_neg(uint2 a, uint2 b, acc_t c) {
        double da = __hiloint2double((int)a.y, (int)a.x);
        double db = __hiloint2double((int)b.y, (int)b.x);
        return __builtin_amdgcn_mfma_f64_16x16x4f64(da, db, c, 0, 0, 1);
    }
};

template <> struct Mx<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static constexpr int EPC = 4;
    static constexpr int EPS = 2;
    // C/D map of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 (lane >> 4) + r
    static __device__ __forceinline__ int crow(int lane, int r) { return 4 * (lane >> 4) + r; }
    static __device__ __forceinline__ uint2 neg(uint2 a) { a.x ^= 0x80000000u; a.y ^= 0x80000000u; return a; }
    static __device__ __forceinline__ acc_t mma(uint2 a, uint2 b, acc_t c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        return c;
    }
    // c - a b (the FP32 instruction has no operand negation: its last field selects lane groups): flip the sign bits
    static __device__ __forceinline__ acc_t mma_neg(uint2 a, uint2 b, acc_t c) { return mma(neg(a), b, c); }
};

template <typename T>
static __device__ __forceinline__ typename Mx<T>::acc_t acc_zero() {
    typename Mx<T>::acc_t z = {0, 0, 0, 0};
    return z;
}

// ------------------------------------------------------- LDS-only barriers ----
// lds_barrier: waits for this wave's LDS traffic, not for global stores in flight (a plain __syncthreads() also
// drains vmcnt, i.e. every store's round trip).  A real fence pair restricted to the LDS address space around
// s_barrier, NOT inline assembly (round 4): the instructions are the same (s_waitcnt lgkmcnt(0); s_barrier), but the
// compiler does not treat an assembly statement's "memory" clobber as an access to __shared__ arrays whose address
// never leaves the kernel -- it kept a value read from LDS two barriers earlier in registers across such a statement
// (potrf.hip, the pivot loop) and may move LDS accesses across one.  Fences are what __syncthreads() is made of and
// do order such accesses.
static __device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// lds_settle: a wave that has just WRITTEN words other waves will read behind the next barrier reads one of them back
// first (the last one it wrote, or any LDS word: the LDS executes one wave's accesses in issue order, so the load's
// data can only return once every earlier store of the wave has been performed).  Round 5: measured on gfx950 with a
// second workgroup on the compute unit (HISTORY.md, round 5): the LAST one or two ds_write
// instructions a wave issued ahead of `s_waitcnt lgkmcnt(0); s_barrier` were not yet in the LDS array when another
// wave's ds_read, issued right behind the barrier, read their words -- it got, bit for bit, what the words held before
// (1.7-3 % of panel chains beside an FP32 trailing update; 0 of 1999 with the read-back).  The wait for a STORE's
// lgkmcnt does not imply visibility to other waves there; the wait for a LOAD's data does.
template <typename T>
static __device__ __forceinline__ void lds_settle(const T* written)
{
    const volatile T* p = written;
    const T v = *p;
    asm volatile("" :: "v"(v));          // the value is "used": the wait for it stays ahead of whatever follows
}

// Zero the elements of a 16-byte chunk whose k index is >= kvalid.
template <typename T>
static __device__ __forceinline__ uint4 mask_chunk(uint4 v, int kfirst, int kvalid);
template <>
__device__ __forceinline__ uint4 mask_chunk<double>(uint4 v, int kfirst, int kvalid) {
    if (kfirst     >= kvalid) { v.x = 0; v.y = 0; }
    if (kfirst + 1 >= kvalid) { v.z = 0; v.w = 0; }
    return v;
}
template <>
__device__ __forceinline__ uint4 mask_chunk<float>(uint4 v, int kfirst, int kvalid) {
    if (kfirst     >= kvalid) v.x = 0;
    if (kfirst + 1 >= kvalid) v.y = 0;
    if (kfirst + 2 >= kvalid) v.z = 0;
    if (kfirst + 3 >= kvalid) v.w = 0;
    return v;
}

// Flip the sign of every element of a 16-byte chunk.
template <typename T> static __device__ __forceinline__ uint4 neg_chunk(uint4 v);
template <> __device__ __forceinline__ uint4 neg_chunk<double>(uint4 v) { v.y ^= 0x80000000u; v.w ^= 0x80000000u; return v; }
template <> __device__ __forceinline__ uint4 neg_chunk<float>(uint4 v)
{
    v.x ^= 0x80000000u; v.y ^= 0x80000000u; v.z ^= 0x80000000u; v.w ^= 0x80000000u;
    return v;
}

// ---------------------------------------------------------------- knobs ----
// Thresholds of the factorisation's schedule.  In the product build these are the constants below and
// nothing reads the environment.  Built with -DCIMRGP_TUNING (tools/build_tuning.sh: the measurement
// builds behind profiles/ and tools/sweep_*.sh) each CIMRGP_* environment variable named here overrides
// its default once, at the first use.
struct Knobs {
    int64_t tail_below = 4864;             // CIMRGP_TAIL_BELOW: trailing matrix at or below this: finish on one queue
    int64_t rows_start_below = 6144;       // CIMRGP_ROWS_START: carried rows start once the trailing matrix is smaller
    int64_t rows_start_below_early = 5632; // CIMRGP_ROWS_START_EARLY: ... in a factorisation that started with early panels (round 5, one box: 6144 / 5632 -> 144.1 / 145.4, 144.5 / 145.1, 144.3 / 145.2; a lone factorisation: 136.8 / 134.4 the other way)
    int64_t far_pair_above = 8192;         // CIMRGP_FAR_PAIR: far part updated once per group of panels above this
    int gemm_pers = 256;                   // CIMRGP_GEMM_PERS: persistent trailing update on at most this many compute units (0: off)
    int pers_min_tiles = 512;              // CIMRGP_PERS_MIN_TILES: 128-tiles below which the tile-per-workgroup kernel is used
    int64_t rows_pair_above = 8192;        // CIMRGP_ROWS_PAIR: the carried rows' far updates take two panels at a time (K = 512) while more columns remain
    int64_t fused_max_chain_wgs = 768;     // CIMRGP_FUSED_MAX: one-queue sweeps ride their updates in the chain's launches while batch x n / 32 is at most this
    int batch_halves_min = 8;              // CIMRGP_BATCH_HALVES: a batched factorisation of at least this many blocks (that does not ride) runs as two halves on two queues
    int rider_round_us = 25;               // CIMRGP_RIDER_ROUND: modelled duration of one round of K = 256 rider tiles (us)
    int rows_cus = 192;                    // CIMRGP_ROWS_CUS: compute units of the carried rows' far updates (persistent kernel; 0: tile-per-workgroup kernel).
                                           // Round 5, one box (profiles/r05_knob_scan.txt): 128 / 160 / 176 / 192 / 208 / 224 / 256 -> 132.0 / 135.8 / 135.8 / 136.8 / 135.4 / 133.4 /
                                           // 130.4 posteriors/s -- two persistent workgroups fill a unit's LDS, and the chain's workgroups need units that hold at most one
    int64_t rows_beside_tail_below = 2560; // CIMRGP_ROWS_BESIDE: with carried rows, the factorisation's tail (trailing matrix at most this) is the one-queue fused sweep while the rows keep their own queues (0: look-ahead to the end)
    int tail_far_cus = 160;                // CIMRGP_TAIL_FAR_CUS: compute units of FAR(prev) on the second queue of the fused tail (0: always riders)
    int64_t tail_far_min_rows = 2048;      // CIMRGP_TAIL_FAR_MIN: ... while at least this many rows remain beyond the next panel
    int chain_cus = 32;                    // CIMRGP_CHAIN_CUS: compute units the bulk update leaves to the panel chain (look-ahead phase)
    int pers_max_chunks = 2;               // CIMRGP_PERS_CHUNKS: the persistent update takes K up to this many panels (256 columns each) in one pass per tile (1: K = 256 only, as in rounds 3-4;
                                           // round 5, one box: potrf n = 12 288 / 16 384 13.80 / 28.51 -> 13.45 / 27.79 ms with 2-3; n = 32 768, whose groups are K = 768: 191.8 -> 200.1 ms with 3 -- so 2)
    int early_panels = 8;                  // CIMRGP_EARLY_PANELS: a staged call whose front end ran on the context's chain queue factors its first panel there, in queue order,
                                           // and this many further panels (update + next panel) one-queue style on the chain queue before the
                                           // look-ahead schedule takes over.  Round 5, one box (profiles/r05_early_panels.txt): 0 / 2 / 4 / 6 / 8 / 10 / 12 / 14 ->
                                           // 137.7 / 139.8 / 140.5 / 143.1 / 143.6 / 143.8 / 141.5 / 138.8 posteriors/s
    int early_cus = 256;                   // CIMRGP_EARLY_CUS: compute units of those early updates (0: the look-ahead phase's share; no chain of their own factorisation runs beside them: 224 -> 256: 144.4 -> 145.0, 145.1 -> 146.1)
};
const Knobs& knobs();
// Queues for the carried rows of cimrgp_potrf_rows (1 or 2): cimrgp_set_rows_queues in include/cimrgp.h.
int rows_queues();
// Pairs of full panels the backward solve takes in one step (build_invT builds their off-diagonal inverse blocks,
// potrs_run uses them): a rule of n alone, so that the factorisation and the solve agree without any state.
static inline int64_t bwd_pairs(int64_t n) { return (n > 5120) ? (n / CIMRGP_NB) / 2 : 0; }
// (potrf.hip) the look-ahead context's queue that is idle between two factorisations on st: cimrgp_solve_queue
hipStream_t solve_queue_for(hipStream_t st);
// (potrf.hip) the context's queue that falls idle before a factorisation on st ends: cimrgp_front_queue
hipStream_t front_queue_for(hipStream_t st);

// ------------------------------------------------ a layer's batch of blocks ----
// The operands every per-layer call passes around (strides in elements).  U is T or const T.
// `batch` matrices of pitch ld, `stride` apart
template <typename U> struct Arena { U* p = nullptr; int64_t ld = 0, stride = 0; };
// one side of a batch: block b is the n rows of x from row starts[b] (NULL: one block at row 0)
template <typename T> struct Points { const T* x = nullptr; const int64_t* starts = nullptr; int64_t n = 0; };
// what both sides share: the number of blocks, the input dimension and the covariance
struct BatchCov { int batch = 1; int d = 0; int cov = CIMRGP_COV_RBF; double ell = 0, sf2 = 0; };
// the blocks' Cholesky factors and the factorisation's workspaces (potrf.hip), sws apart
template <typename U> struct Factors { Arena<U> l; U* ws = nullptr; int64_t sws = 0; };
// where the inverted 256 x 256 diagonal panels start in a factorisation workspace: behind the ceil(n / 64) inverted
// 64 x 64 blocks (potrf.hip, build_invT)
static inline int64_t ws_invT_offset(int64_t n) { return (n + 63) / 64 * (64 * 64); }

// --------------------------------------------------------- host launchers ----
// block.hip: the three stages of cimrgp_block_posterior[_staged] on their streams, with the records of staged calls
// in flight; staged_shutdown_ destroys those records' events (cimrgp_shutdown)
template <typename T> int block_posterior_typed(const void* x, int64_t n, int d, const void* y, int q, const void* xs, int64_t ns,
                                                double ell, double sf2, double noise, void* k, int64_t ldk, void* ws, int32_t* info,
                                                void* w, int64_t ldw, void* alpha, void* z, void* scratch, void* mean, void* var,
                                                int add_noise, int accumulate, hipStream_t s_front, hipStream_t st, hipStream_t s_solve);
int staged_shutdown_();
// potrf.hip
template <typename T> int potrf_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb,
                                    hipStream_t st, hipStream_t ready_on = nullptr);
// `batch` equal-sized factorisations in the same launches (strides in elements / ints)
struct PotrfBatch { int count = 1; int64_t sk = 0, sws = 0, sb = 0; };
// `count` factors f with carried rows (or right-hand sides) sb apart
template <typename U> static inline PotrfBatch potrf_batch(int count, const Factors<U>& f, int64_t sb) { return PotrfBatch{count, f.l.stride, f.sws, sb}; }
template <typename T> int potrf_batched_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb,
                                            PotrfBatch bt, hipStream_t st);
template <typename T> int solve_rows_run(const T* l, int64_t n, int64_t ld, const T* ws, T* b, int64_t m,
                                         int64_t ldb, hipStream_t st, PotrfBatch bt = PotrfBatch());
int potrf_shutdown();     // destroys the look-ahead contexts (streams, events): cimrgp_shutdown
int profile_begin();
int profile_pause();
int profile_collect(double* total_ms, double* total_flops, int64_t* launches, double* total_bytes = nullptr);
// gemm_nt.hip
// A batch of independent products in one launch (equal shapes; element strides between problems).
// skip_first: the first 64 x 64 tile of a rectangular update is left alone (the chain has already
// replaced it by its factor; only honoured when the launch uses 64-tiles: gemm_uses_tile64)
// pers: compute units for the persistent form of the update (-1: knobs().gemm_pers, 0: never)
// head_first + flag: the look-ahead's combined head + bulk update as one persistent launch (gemm_nt.hip)
struct GemmBatch { int count = 1; int64_t sc = 0, sa = 0, sb = 0; int skip_first = 0; int pers = -1; int head_first = 0; int* flag = nullptr; int pers_force = 0; };
static inline GemmBatch gemm_batch(int count, int64_t sc, int64_t sa, int64_t sb) { GemmBatch g; g.count = count; g.sc = sc; g.sa = sa; g.sb = sb; return g; }
bool gemm_uses_tile64(int64_t m, int64_t n, bool lower, int count = 1);
int gemm_pers_head_tiles(int64_t m, int k, int elem_bytes);
template <typename T> int gemm_nt_sub(T* c, int64_t ldc, const T* a, int64_t lda, const T* b, int64_t ldb,
                                      int64_t m, int64_t n, int k, bool lower, hipStream_t st, GemmBatch bt = GemmBatch());

// ------------------------------------------------------ covariance policies ----
// The stationary covariances of the dense path (CIMRGP_COV_*, include/cimrgp.h), as functions of the squared distance
// d2 = sum_k (x_k - x'_k)^2.  `c` is the policy's scale, fixed on the host by cov_scale(): RBF -1 / (2 l^2) (the
// expression the RBF kernels always used, so that their results stay bit-identical), Matern sqrt(2 nu) / l, so that
// t = c r.  r = |df| for one input dimension, sqrt(d2) otherwise: d2 is a sum of squares, so it is exactly 0 on the
// diagonal and never negative.
static inline bool cov_known(int cov) { return cov >= CIMRGP_COV_RBF && cov <= CIMRGP_COV_MATERN52; }

static inline double cov_scale(int cov, double ell)
{
    switch (cov) {
        case CIMRGP_COV_MATERN12: return 1.0 / ell;
        case CIMRGP_COV_MATERN32: return sqrt(3.0) / ell;
        case CIMRGP_COV_MATERN52: return sqrt(5.0) / ell;
        default: return -0.5 / (ell * ell);
    }
}

// The one run-time -> compile-time dispatch over the policies: f(std::integral_constant<int, COV>) for the id `cov`
// (validated by the entry points; anything else takes the RBF).
template <typename F> static inline int with_cov(int cov, F&& f)
{
    switch (cov) {
        case CIMRGP_COV_MATERN12: return f(std::integral_constant<int, CIMRGP_COV_MATERN12>());
        case CIMRGP_COV_MATERN32: return f(std::integral_constant<int, CIMRGP_COV_MATERN32>());
        case CIMRGP_COV_MATERN52: return f(std::integral_constant<int, CIMRGP_COV_MATERN52>());
        default: return f(std::integral_constant<int, CIMRGP_COV_RBF>());
    }
}

// The other run-time -> compile-time dispatches of the covariance code, in the same form.
// with_dim: the input dimension as D = 1, 2 or 0 (0: run-time d <= MAXD, fully unrolled and predicated loops)
template <typename F> static inline auto with_dim(int d, F&& f)
{
    if (d == 1) return f(std::integral_constant<int, 1>());
    if (d == 2) return f(std::integral_constant<int, 2>());
    return f(std::integral_constant<int, 0>());
}
// with_q: the number of outputs (right-hand sides) as Q = q exactly, 1 .. MAXQ (validated by the entry points)
template <typename F> static inline auto with_q(int q, F&& f)
{
    switch (q) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
        case 7: return f(std::integral_constant<int, 7>());
        default: return f(std::integral_constant<int, 8>());
    }
}
// with_q_rounded: Q = q up to 4, then 8 for kernels that guard c < q at run time (half the instances)
template <typename F> static inline auto with_q_rounded(int q, F&& f)
{
    switch (q) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        default: return f(std::integral_constant<int, 8>());
    }
}

// Tile id of the lower triangle (row-major: id = ti (ti + 1) / 2 + tj, tj <= ti) -> (ti, tj)
static __device__ __forceinline__ void lower_tile_of(int id, int& ti, int& tj)
{
    ti = (int)((sqrtf(8.0f * (float)id + 1.0f) - 1.0f) * 0.5f);
    while (ti * (ti + 1) / 2 > id) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
    tj = id - ti * (ti + 1) / 2;
}

// Every policy has value(d2, df0, c, sf2) = k and pair(d2, df0, c, sf2, k, g, dl), what the derivative kernels need of
// one pair of points: k, g with dk/da_e = -g (a_e - b_e), and dl = dk / dlog l.  df0 is the first difference: the
// Matern policies take r = |df0| when D = 1.
template <int COV> struct Cov;

template <> struct Cov<CIMRGP_COV_RBF> {
    template <typename T, int D> static __device__ __forceinline__ T value(T d2, T, T c, T sf2) { return sf2 * exp(d2 * c); }
    template <typename T, int D> static __device__ __forceinline__ void pair(T d2, T df0, T c, T sf2, T& k, T& g, T& dl)
    {
        k = value<T, D>(d2, df0, c, sf2);
        g = k * ((T)-2 * c);
        dl = g * d2;
    }
};

// Matern policies: value(d2) and, for the gradient of the log marginal likelihood w.r.t. log l,
//   dlogl = -r dk/dr  (isotropic: d k / d log l)
//   ard   = -(dk/dr) / r  (per dimension with pre-scaled inputs: d k / d log l_k = ard * (x_k - x'_k)^2; it is also g)
// both finite at r = 0 except ard for nu = 1/2, which is defined as 0 there (every (x_k - x'_k)^2 is 0 too).
template <int COV> struct MaternCov {
    template <typename T> static __device__ __forceinline__ T poly(T t)
    {
        if (COV == CIMRGP_COV_MATERN12) return (T)1;
        if (COV == CIMRGP_COV_MATERN32) return (T)1 + t;
        return (T)1 + t + t * t * (T)(1.0 / 3.0);
    }
    template <typename T, int D> static __device__ __forceinline__ T radius(T d2, T df0) { return D == 1 ? fabs(df0) : sqrt(d2); }
    template <typename T, int D> static __device__ __forceinline__ T value(T d2, T df0, T c, T sf2)
    {
        const T t = c * radius<T, D>(d2, df0);
        return sf2 * poly(t) * exp(-t);
    }
    // t = c r, v = exp(-t)
    template <typename T> static __device__ __forceinline__ T dlogl(T t, T v, T sf2)
    {
        if (COV == CIMRGP_COV_MATERN12) return sf2 * t * v;
        if (COV == CIMRGP_COV_MATERN32) return sf2 * t * t * v;
        return sf2 * t * t * ((T)1 + t) * v * (T)(1.0 / 3.0);
    }
    template <typename T> static __device__ __forceinline__ T ard(T t, T r, T v, T c, T sf2)
    {
        if (COV == CIMRGP_COV_MATERN12) return r > (T)0 ? sf2 * c * v / r : (T)0;
        if (COV == CIMRGP_COV_MATERN32) return c * c * sf2 * v;
        return c * c * sf2 * ((T)1 + t) * v * (T)(1.0 / 3.0);
    }
    template <typename T, int D> static __device__ __forceinline__ void pair(T d2, T df0, T c, T sf2, T& k, T& g, T& dl)
    {
        const T r = radius<T, D>(d2, df0);
        const T t = c * r;
        const T v = exp(-t);
        k = sf2 * poly(t) * v;
        g = ard(t, r, v, c, sf2);
        dl = dlogl(t, v, sf2);
    }
};
template <> struct Cov<CIMRGP_COV_MATERN12> : MaternCov<CIMRGP_COV_MATERN12> {};
template <> struct Cov<CIMRGP_COV_MATERN32> : MaternCov<CIMRGP_COV_MATERN32> {};
template <> struct Cov<CIMRGP_COV_MATERN52> : MaternCov<CIMRGP_COV_MATERN52> {};

// gram.hip.  cov: CIMRGP_COV_* (validated by the caller); fn: the entry point named in error messages (NULL: the RBF
// entry point's name); lin: d FP64 weights on the device, every element gets + sum_e lin[e] xa_ie xb_je (nullptr: no such term)
template <typename T> int rbf_gram_run(const T* xa, int64_t na, const T* xb, int64_t nb, int d, double ell, double sf2,
                                       double diag_add, T* k, int64_t ld, bool symm, bool lower_only, hipStream_t st,
                                       int cov = CIMRGP_COV_RBF, const char* fn = nullptr, const double* lin = nullptr);
// K_b = k(rows_b, cols_b) for every block b into arena k; symm: rows == cols, the lower tiles, + diag_dev[b] on the diagonal
template <typename T> int rbf_gram_batched_run(const BatchCov& bc, const Points<T>& rows, const Points<T>& cols, const T* diag_dev,
                                               const Arena<T>& k, bool symm, hipStream_t st);
template <typename T> int predict_mean_run(const T* x, int64_t n, int d, const T* alpha, int q, const T* xs, int64_t ns,
                                           double ell, double sf2, const T* bias, T* mean, int accumulate, hipStream_t st,
                                           int cov = CIMRGP_COV_RBF, const char* fn = nullptr);
// solve.hip
template <typename T> int potrs_run(const T* l, int64_t n, int64_t ld, const T* ws, T* rhs, int q, T* z_out, T* scratch,
                                    bool backward_only, hipStream_t st, PotrfBatch bt = PotrfBatch(), bool work_ready = false);
template <typename T> int predict_from_w_run(const T* w, int64_t ns, int64_t n, int64_t ldw, const T* z, int q, double sf2,
                                             double extra, const T* extra_dev, const T* bias, T* mean, T* var, int accumulate,
                                             hipStream_t st, int batch = 1, const int64_t* t_starts = nullptr, int64_t sw = 0);
// misc.hip
template <typename T> int misc_block_stats(const T* y, const T* fbar, int64_t n, int q, T* stats, hipStream_t st);
template <typename T> int misc_residual(const T* y, const T* fbar, const T* bias, int64_t n, int q, T* r, hipStream_t st);
template <typename T> int misc_train_mean(const T* r, const T* alpha, const T* bias, const T* noise, int64_t n, int q,
                                          T* out, int accumulate, hipStream_t st);
template <typename T> int misc_add_diag(T* k, int64_t n, int64_t ld, const T* noise, hipStream_t st);
template <typename T> int misc_noise_from_stats(const T* stats, int q, double frac, double floor_value, T* noise, hipStream_t st);
template <typename T> int misc_logdet_half(const T* l, int64_t n, int64_t ld, double* out, hipStream_t st);
template <typename T> int lml_grad_run(const T* x, int64_t n, int d, const T* kinv, int64_t ld, const T* alpha, int q,
                                       double ell, double sf2, double noise, double* out3, double* scratch, hipStream_t st,
                                       bool ard = false, int cov = CIMRGP_COV_RBF, const char* fn = nullptr);
// the gradient of `batch` blocks (K^-1 lower triangles at ks apart, inputs from rows starts[b]) and each block's log
// marginal likelihood from its factor l (same layout as kinv) and z = L^-1 r (batch x n x q): out[4 b + 0 .. 3];
// partial: batch x lml_grad_tiles_count(n) x lml_grad_record_width(ard) doubles.  ard: x pre-scaled by the length-scales,
// unit length-scale (ell is not read), d length-scale entries: out[(d + 3) b + 0 .. d + 2]
int64_t lml_grad_tiles_count(int64_t n);
int lml_grad_record_width(bool ard);
template <typename T> int lml_grad_batched_run(const T* x, const int64_t* starts, int batch, int64_t n, int d, const T* kinv,
                                               int64_t ld, int64_t ks, const T* l, const T* alpha, const T* z, int q, double ell,
                                               double sf2, double noise, double* out, double* partial, hipStream_t st, int cov,
                                               const char* fn, bool ard = false);

// layer.hip: one call per layer for a batch of equal-sized blocks
// The fit front end (fit_front_run): statistics -> bias, noise | residual rows | Gram + noise | factorisation with the
// rows carried | z | backward solve (alpha).  f.l holds the Gram matrices, then the factors.
template <typename T> struct FitFront {
    BatchCov bc; Points<T> tr; Factors<T> f; int32_t* info = nullptr;
    const T* y = nullptr; const T* fbar = nullptr; int q = 0; const T* shared_bias = nullptr;
    // noise[b]: the fixed value if >= 0, else the shared one if given, else max(frac var, floor)
    double noise_fixed = 0, noise_frac = 0, noise_floor = 0; const T* shared_noise = nullptr;
    Arena<T> rows; bool eye = false;     // the carried rows: q residual rows per block, then (eye) the n rows of the identity
    T* z = nullptr; T* alpha = nullptr; T* work = nullptr; T* bias = nullptr; T* noise = nullptr;   // work: potrs_run's scratch
};
template <typename T> struct LayerFit { FitFront<T> fr; T* train_out = nullptr; };
template <typename T> int layer_fit_run(const LayerFit<T>& a, hipStream_t st);
// W_b = K(tests_b, train_b) L_b^-T into arena w: the cross-Gram, then the row solve (predict, joint covariance, gradient)
template <typename T> int cross_solve_run(const BatchCov& bc, const Points<T>& train, const Factors<const T>& f, const Points<T>& tests,
                                          const Arena<T>& w, hipStream_t st);
template <typename T> struct LayerPredict {
    BatchCov bc; Points<T> tr; Factors<const T> f; Points<T> te;
    const T* z = nullptr; int q = 0; const T* bias = nullptr; const T* noise = nullptr;
    Arena<T> w; T* mean = nullptr; T* var = nullptr;
};
template <typename T> int layer_predict_run(const LayerPredict<T>& a, hipStream_t st);
// joint.hip: c.l = the covariance blocks, factored in place with the workspaces c.ws when those are given
template <typename T> struct LayerJoint {
    BatchCov bc; Points<T> tr; Factors<const T> f; Points<T> te;
    const T* diag = nullptr; Arena<T> w; Factors<T> c; int32_t* info = nullptr;
};
// grad.hip: alpha_b at alpha + b sa; w: the work area of the layer call (its beta), or the caller's beta (single block)
template <typename T> struct LayerGrad {
    BatchCov bc; Points<T> tr; Factors<const T> f; Points<T> te;
    const T* alpha = nullptr; int64_t sa = 0; int q = 0; Arena<T> w; T* mg = nullptr; T* vg = nullptr; int accumulate = 0;
};
// log marginal likelihood + gradient of a batch of blocks (cimrgp_layer_lml_grad_cov and its ARD twin); the scratch holds the carried
// rows (q residual rows + the identity, per block), z, alpha, the backward solve's work area, bias, noise and the
// gradient's tile records, at the byte offsets of lml_scratch_layout: layer_lml_grad_run points fr's rows, z, alpha,
// work, bias and noise there (fr.noise_fixed is the call's noise).  np: entries per tile record (lml_grad_record_width)
struct LmlScratch { int64_t ldr = 0, srows = 0; size_t rows = 0, z = 0, alpha = 0, work = 0, bias = 0, noise = 0, partial = 0, total = 0; };
LmlScratch lml_scratch_layout(size_t esz, int64_t n, int q, int batch, int np);
template <typename T> struct LayerLml { FitFront<T> fr; T* kinv = nullptr; void* scratch = nullptr; double* out = nullptr; };
template <typename T> int layer_lml_grad_run(const LayerLml<T>& a, hipStream_t st, bool ard);

// reduced.hip
template <typename T> int laplace_basis_run(const T* x, int64_t n, int d, const double* interval, int m, T* phi, hipStream_t st);
int basis_moments_workgroups(int64_t n);
template <typename T> int basis_moments_run(const T* x, int64_t n, int d, const double* interval, int m, const T* y, const T* fbar,
                                            const T* fvar, const double* eau, int q, double* out, double* scratch, hipStream_t st);
template <typename T> int basis_apply_run(const T* x, int64_t n, int d, const double* interval, int m, const double* eau, int q,
                                          const double* bias, const double* c2, double bias_var, T* mean, T* var, int accumulate,
                                          hipStream_t st);

}  // namespace cimrgp
