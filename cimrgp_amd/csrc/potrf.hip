// Blocked right-looking Cholesky (lower, row-major, in place) and the row-wise
// triangular solve that shares its panel kernels.
//
//   for each panel of CIMRGP_NB = 256 columns:
//     for each 64-column sub-block s of the panel (left-looking inside the panel):
//        k_diag64   one workgroup: A_ss -= L_s,prev L_s,prev^T (MFMA), factor the
//                   64x64 block from registers and form its inverse alongside
//        k_trsm64   rows below: X = (P_s - P_prev L_s,prev^T) inv(L_ss)^T  (MFMA, in place)
//     gemm_nt (lower)  trailing matrix -= panel * panel^T       (MFMA, K = 256)
//
// The inverted 64x64 diagonal blocks stay in the workspace (slab c0/64) and
// are what cimrgp_potrs / cimrgp_trsm_rows use afterwards.
//
// The kernels are in chain_kernels.hpp (the panel chain and its riders) and rows_kernels.hpp (carried
// rows, inverses, the gate); this file is the host schedule that launches them.
#include "common.hpp"
#include "chain_kernels.hpp"
#include "rows_kernels.hpp"
#include <cstdlib>
#include <functional>
#include <mutex>
#include <vector>

namespace cimrgp {

// ---- optional per-launch timing of the trailing update (bench.py roofline) ----
// Events are recorded on the launch stream around every lower-triangular
// trailing-update launch while profiling is on; collect() waits for them.
namespace {
struct TrailRec { hipEvent_t start, stop; double flops, bytes; };
std::vector<TrailRec> g_recs;
std::vector<TrailRec> g_free;
bool g_profile = false;
std::mutex g_profile_mutex;            // factorisations on different caller streams may be enqueued by different host threads
}  // namespace

int profile_begin()
{
    std::lock_guard<std::mutex> guard(g_profile_mutex);
    g_profile = true;
    return 0;
}

// Stops recording without touching the records so far (profile_begin resumes): bench.py brackets the launches of
// every fourth step only -- two event records per launch on the update queue cost ~1 % of an N = 8192 step.
int profile_pause()
{
    std::lock_guard<std::mutex> guard(g_profile_mutex);
    g_profile = false;
    return 0;
}

int profile_collect(double* total_ms, double* total_flops, int64_t* launches, double* total_bytes)
{
    std::lock_guard<std::mutex> guard(g_profile_mutex);
    double ms = 0.0, fl = 0.0, by = 0.0;
    int64_t cnt = 0;
    for (auto& r : g_recs) {
        hipError_t e = hipEventSynchronize(r.stop);
        if (e != hipSuccess) return check_hip(e, "cimrgp_profile_collect", "hipEventSynchronize");
        float t = 0.f;
        e = hipEventElapsedTime(&t, r.start, r.stop);
        if (e != hipSuccess) return check_hip(e, "cimrgp_profile_collect", "hipEventElapsedTime");
        ms += t; fl += r.flops; by += r.bytes; ++cnt;
        g_free.push_back(r);
    }
    g_recs.clear();
    g_profile = false;
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    if (total_bytes) *total_bytes = by;
    if (launches) *launches = cnt;
    return 0;
}

// Opens a record (start event on `st`) and returns its stop event, to be recorded behind the launch;
// nullptr when profiling is off.
// flops = M (M + 1) K of a lower update; bytes = its algorithmic traffic: C (lower) read and written, the panel once
static hipEvent_t rec_open(hipStream_t st, double flops, double bytes = 0.0)
{
    std::lock_guard<std::mutex> guard(g_profile_mutex);
    if (!g_profile) return nullptr;
    TrailRec r;
    if (!g_free.empty()) { r = g_free.back(); g_free.pop_back(); }
    else {
        if (hipEventCreate(&r.start) != hipSuccess || hipEventCreate(&r.stop) != hipSuccess) return nullptr;
    }
    r.flops = flops;
    r.bytes = bytes;
    (void)hipEventRecord(r.start, st);
    g_recs.push_back(r);
    return r.stop;
}

namespace {

// Far part of the trailing matrix updated once per group of panels while larger than this.
// Measured: whole potrf at N = 65536 1650 -> 1505 ms (56.9 -> 62.3 TF/s); at N = 8192 pairing
// (thresholds 2048..6144) raises the update kernel's rate (49 -> 56 % of peak) but not the
// end-to-end time (longer-lived update workgroups, longer slot waits of the chain), so it
// starts above that size.

constexpr int64_t ROWS_PAIR_ABOVE_SOLVE = 1024;   // stand-alone row-wise solve: pair the updates while more columns remain

// (the schedule's thresholds are `knobs()`, common.hpp: constants in the product build)

}  // namespace

// One pass over the panels.  With FACTOR the matrix itself is factored; with
// rows (b != nullptr) the extra rows are carried through the same panel
// operations, which turns them into  B L^-T.
// How many panels share one pass over the far part of the matrix being updated (K = 256 x that
// many).  Stand-alone rate of the update at K = 256 / 512 / 768 / 1024: 51.5 / 59.0 / 62.1 / 63.5
// TF/s at M = 15360, 55.5 / 62.1 / 64.3 / 65.3 TF/s at M = 32256.  Inside the factorisation
// (whole potrf, groups capped at 1 / 2 / 3 / 4): N = 32768: 217.8 / 203.9 / 201.3 / 200.9 ms,
// N = 65536: 1650 / 1512 / 1505 / 1505 ms -- pairs bring most of it.  The group is also kept
// small enough for the operand panel (far x K x 8 bytes) to fit the 256 MB Infinity Cache, which
// caps it at 3 (a group of 4 would need far > 32768 and far <= 32768 at once).
static inline int group_size(int64_t far, int64_t pair_above)
{
    if (far <= pair_above) return 1;
    const int by_benefit = (far > 16384) ? 3 : 2;
    const int64_t by_cache = ((int64_t)1 << 17) / far;       // 2^28 bytes / (8 bytes x far rows x 256 columns)
    const int g = (by_cache < by_benefit) ? (int)by_cache : by_benefit;
    return g < 1 ? 1 : g;
}

struct PanelGroup {
    int64_t g0 = -1;      // first column of the group's first panel (-1: no group open)
    int left = 0;         // panels of the group still to come, this one included
    bool near_pending = false;   // carried rows: the previous panel's update of THIS panel's columns is owed (k_rows_step applies it)
};

// The latency-bound chain of one panel [k0, k0 + w) on stream st: the first 64-column diagonal
// block in a launch of its own, then one k_link per further sub-block (panel solve of sub-block s
// beside the factorisation of diagonal block s + 1), and the panel solve of the last sub-block.
// b (m x .., leading dimension ldb): carried rows solved along (second row set), or nullptr.
// `alone`: nothing heavy runs beside the chain (one-queue sweeps, the tail).  Then the nine-wave
// kernels are used (a few per cent faster by themselves: N = 2048 1.05 against 1.09 ms).  Beside a
// running trailing update a nine-wave workgroup is dispatched only to a compute unit BOTH of whose
// update workgroups have retired -- in effect after the update's last generation (first link of a
// panel 230-300 us at N = 8192) -- while a four-wave workgroup fits beside one update workgroup and
// gets, by queue priority, the first slot that falls free: there the four-wave forms run
// (N = 8192: period of the update-bound panels 437 / 391 / 371 -> 405 / 363 / 355 us).
// `riders`: nullptr, or the update tiles riding in the chain's launches -- riders[0] in the first diagonal
// block's launch, riders[1..3] in the links, riders[4] in the last sub-block's panel solve (fused_sweep).
// `left64`: the first diagonal block takes, as its left-looking prologue, the 64 columns just left of the
// panel (the previous panel's last sub-block, whose contribution the riders could not apply before it was final).
template <typename T>
static int panel_chain(T* kmat, int64_t n, int64_t ld, T* ws, int32_t* info, int64_t k0, int64_t w,
                       T* b, int64_t m, int64_t ldb, PotrfBatch bt, hipStream_t st, const char* fn, bool alone,
                       bool first_done = false, const Riders<T>* riders = nullptr, bool left64 = false)
{
    // (a batch of factorisations in one launch is its own crowd: many link workgroups compete for the
    // compute units, and the four-wave form packs twice as many of them)
    const bool waves4 = !alone || bt.count > 1;
    const bool rows = (b != nullptr && m > 0);
    const unsigned nbatch = (unsigned)bt.count;
    const int64_t k1 = k0 + w;
    // rows per panel-solve workgroup: groups of TRSM_GROUP tiles in batched launches (k_linkq / k_trsm64 take it as an argument)
    const int trg = (bt.count > 1 && waves4) ? TR * TRSM_GROUP : TR;
    const int nb2 = rows ? (int)((m + trg - 1) / trg) : 0;
    const Riders<T> none = no_riders<T>();
    int launch = 0;                                   // 0: first diagonal block, 1..3: links, 4: last panel solve
    for (int64_t c0 = k0; c0 < k1; c0 += SB) {
        const int sw = (int)((k1 - c0 < SB) ? (k1 - c0) : SB);
        const int kprev = (int)(c0 - k0);
        const int64_t pc = c0 + sw;            // first row after this sub-block
        T* inv = ws + (c0 / SB) * (SB * SB);
        const T* lrow = kmat + c0 * ld + k0;   // rows of the diagonal block, earlier panel columns
        if (c0 == k0 && !first_done) {
            const Riders<T>& rd = (riders && c0 == k0) ? riders[0] : none;
            const bool l64 = left64 && c0 == k0;
            const T* lr = l64 ? lrow - SB : lrow;
            const int kp = l64 ? SB : kprev;
            if (waves4)
                hipLaunchKernelGGL((k_diag64q<T>), dim3((unsigned)(1 + rd.total), nbatch), dim3(Q_NT), 0, st,
                                   kmat + c0 * ld + c0, ld, sw, lr, kp, inv, info, (int)c0, bt.sk, bt.sws, bt.sb, rd);
            else
                hipLaunchKernelGGL((k_diag64<T>), dim3((unsigned)(1 + rd.total), nbatch), dim3(DG_NT), 0, st,
                                   kmat + c0 * ld + c0, ld, sw, lr, kp, inv, info, (int)c0, bt.sk, bt.sws, bt.sb, rd);
            CIMRGP_LAUNCH_CHECK(fn);
        }
        if (pc < k1) {
            const int wn = (int)((k1 - pc < SB) ? (k1 - pc) : SB);         // next diagonal block of this panel
            const int64_t m1 = n - (pc + wn);
            const int nb1 = (int)((m1 + (waves4 ? trg : TR) - 1) / (waves4 ? trg : TR));
            ++launch;
            const Riders<T>& rd = (riders && launch <= 3) ? riders[launch] : none;
            const int nchain = 1 + nb1 + nb2;
            if (waves4)
                hipLaunchKernelGGL((k_linkq<T>), dim3((unsigned)(nchain + rd.total), nbatch), dim3(Q_NT), 0, st,
                                   kmat, ld, (int)n, (int)c0, (int)k0, wn, rows ? b + c0 : (T*)nullptr, ldb, rows ? (int)m : 0,
                                   ws, info, bt.sk, bt.sws, bt.sb, nchain, rd, trg);
            else
                hipLaunchKernelGGL((k_link<T>), dim3((unsigned)(nchain + rd.total), nbatch), dim3(DG_NT), 0, st,
                                   kmat, ld, (int)n, (int)c0, (int)k0, wn, rows ? b + c0 : (T*)nullptr, ldb, rows ? (int)m : 0,
                                   ws, info, bt.sk, bt.sws, bt.sb, nchain, rd);
            CIMRGP_LAUNCH_CHECK(fn);
            continue;
        }
        const int64_t m1 = n - pc;
        const int nb1 = (int)((m1 + trg - 1) / trg);
        const Riders<T>& rd = (riders && pc == k1) ? riders[4] : none;
        if (nb1 + nb2 + rd.total > 0) {
            hipLaunchKernelGGL((k_trsm64<T>), dim3((unsigned)(nb1 + nb2 + rd.total), nbatch), dim3(256), 0, st,
                               kmat + pc * ld + c0, ld, (int)m1, nb1,
                               rows ? b + c0 : (T*)nullptr, ldb, rows ? (int)m : 0,
                               sw, kprev, lrow, ld, (const T*)inv, bt.sk, bt.sws, bt.sb, nb1 + nb2, rd, trg);
            CIMRGP_LAUNCH_CHECK(fn);
        }
    }
    return 0;
}

// One panel of a row-wise solve  B <- B L^-T : the 256-wide solve of the panel's columns, then
// the update of the columns right of it.  While more than `pair_above` columns lie beyond the
// next panel, the far columns are updated once per GROUP of panels with K = 256 x group size
// (fewer passes over B): every panel of a group but the last only updates the next panel's
// columns (with all the group's panels so far), the last one everything right of itself
// (adjacent panels are adjacent columns of B and of L).
// The rows' solve of one full panel [r0, r0 + 256): k_rows_step, with the previous panel's update of these columns
// fused in (`with_prev`: the caller left it out of its updates) or as the solve alone.
template <typename T>
static int rows_step_launch(T* b, int64_t ldb, int64_t m, const T* lmat, int64_t ld, const T* ws, int64_t r0, bool with_prev,
                            hipStream_t st, const char* fn, PotrfBatch bt = PotrfBatch())
{
    // (a batch: blockIdx.y = matrix, strides of the rows' arena, the matrices and the workspaces)
    const dim3 grid((unsigned)((m + RowsStep<T>::R - 1) / RowsStep<T>::R), (unsigned)bt.count);
    if (with_prev)
        hipLaunchKernelGGL((k_rows_step<T, true>), grid, dim3(256), 0, st, b + r0, ldb, (int)m,
                           (const T*)(lmat + r0 * ld + (r0 - CIMRGP_NB)), ld, (const T*)(ws + (r0 / SB) * (SB * SB)),
                           (const T*)nullptr, (int64_t)0, 0, 1, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0, bt.sb, bt.sk, bt.sws);
    else
        hipLaunchKernelGGL((k_rows_step<T, false>), grid, dim3(256), 0, st, b + r0, ldb, (int)m,
                           (const T*)(lmat + r0 * ld + r0), ld, (const T*)(ws + (r0 / SB) * (SB * SB)),
                           (const T*)nullptr, (int64_t)0, 0, 1, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0, bt.sb, bt.sk, bt.sws);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

template <typename T>
static int rows_panel_step(T* b, int64_t ldb, int64_t m, const T* lmat, int64_t ld, int64_t n, const T* ws,
                           int64_t r0, PanelGroup& grp, int64_t pair_above, hipStream_t st, const char* fn,
                           PotrfBatch bt = PotrfBatch())
{
    const int64_t rw = (n - r0 < CIMRGP_NB) ? (n - r0) : CIMRGP_NB;
    const int64_t r1 = r0 + rw;
    GemmBatch gb; gb.count = bt.count; gb.sc = gb.sa = bt.sb; gb.sb = bt.sk;
    const bool near_pending = grp.near_pending;
    grp.near_pending = false;
    if (m > 0 && rw == CIMRGP_NB) {
        int rcs = rows_step_launch<T>(b, ldb, m, lmat, ld, ws, r0, near_pending, st, fn, bt);
        if (rcs) return rcs;
    } else {
        if (near_pending) {                      // (cannot happen: the promise below is made for full panels only)
            int rcn = gemm_nt_sub<T>(b + r0, ldb, b + r0 - CIMRGP_NB, ldb, lmat + r0 * ld + r0 - CIMRGP_NB, ld, m, rw, CIMRGP_NB, false, st, gb);
            if (rcn) return rcn;
        }
        hipLaunchKernelGGL((k_trsm256<T>), dim3((unsigned)((m + TR - 1) / TR), (unsigned)bt.count), dim3(256), 0, st,
                           b + r0, ldb, (int)m, (int)rw, (const T*)(lmat + r0 * ld + r0), ld,
                           (const T*)(ws + (r0 / SB) * (SB * SB)), bt.sb, bt.sk, bt.sws);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    if (n <= r1) { grp = PanelGroup(); return 0; }
    const int64_t rn = (n - r1 < CIMRGP_NB) ? (n - r1) : CIMRGP_NB;
    if (grp.g0 < 0) {
        const int g = group_size(n - (r1 + rn), pair_above);
        if (g > 1) { grp.g0 = r0; grp.left = g; }
    }
    if (grp.g0 >= 0 && grp.left > 1 && n > r1 + rn) {
        --grp.left;
        return gemm_nt_sub<T>(b + r1, ldb, b + grp.g0, ldb, lmat + r1 * ld + grp.g0, ld, m, rn, (int)(r1 - grp.g0), false, st, gb);
    }
    const int64_t kk0 = (grp.g0 >= 0) ? grp.g0 : r0;
    grp = PanelGroup();
    if (m > 0 && kk0 == r0 && rw == CIMRGP_NB && rn == CIMRGP_NB) {
        // the next panel's columns take this panel's update inside their own solve (k_rows_step)
        grp.near_pending = true;
        if (n <= r1 + rn) return 0;
        return gemm_nt_sub<T>(b + r1 + rn, ldb, b + r0, ldb, lmat + (r1 + rn) * ld + r0, ld, m, n - (r1 + rn), (int)rw, false, st, gb);
    }
    return gemm_nt_sub<T>(b + r1, ldb, b + kk0, ldb, lmat + r1 * ld + kk0, ld, m, n - r1, (int)(r1 - kk0), false, st, gb);
}

template <typename T, bool FACTOR>
static int panel_sweep(T* kmat, int64_t n, int64_t ld, T* ws, int32_t* info,
                       T* b, int64_t m, int64_t ldb, hipStream_t st, PotrfBatch bt = PotrfBatch())
{
    const char* fn = FACTOR ? "cimrgp_potrf" : "cimrgp_trsm_rows";
    const bool rows = (b != nullptr && m > 0);
    PanelGroup rows_grp;
    for (int64_t k0 = 0; k0 < n; k0 += CIMRGP_NB) {
        const int64_t w = (n - k0 < CIMRGP_NB) ? (n - k0) : CIMRGP_NB;
        const int64_t k1 = k0 + w;
        if (!FACTOR && rows) {
            int rc = rows_panel_step<T>(b, ldb, m, kmat, ld, n, ws, k0, rows_grp, ROWS_PAIR_ABOVE_SOLVE, st, fn, bt);
            if (rc) return rc;
            continue;
        }
        if (FACTOR) {
            int rcc = panel_chain<T>(kmat, n, ld, ws, info, k0, w, b, m, ldb, bt, st, fn, true);
            if (rcc) return rcc;
        }
        if (n > k1) {
            if (FACTOR) {
                const double mm = (double)(n - k1);
                hipEvent_t rec = rec_open(st, mm * (mm + 1.0) * (double)w * (double)bt.count, (mm * (mm + 1.0) + mm * (double)w) * (double)sizeof(T) * (double)bt.count);   // lower SYRK: M(M+1)K flop
                GemmBatch gb; gb.count = bt.count; gb.sc = gb.sa = gb.sb = bt.sk;
                int rc = gemm_nt_sub<T>(kmat + k1 * ld + k1, ld, kmat + k1 * ld + k0, ld,
                                        kmat + k1 * ld + k0, ld, n - k1, n - k1, (int)w, true, st, gb);
                if (rec) (void)hipEventRecord(rec, st);
                if (rc) return rc;
            }
            if (rows) {
                GemmBatch gb; gb.count = bt.count; gb.sc = gb.sa = bt.sb; gb.sb = bt.sk;
                int rc = gemm_nt_sub<T>(b + k1, ldb, b + k0, ldb, kmat + k1 * ld + k0, ld,
                                        m, n - k1, (int)w, false, st, gb);
                if (rc) return rc;
            }
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// One-queue factorisation with the updates riding in the chain's launches (round 3; "Riders" above).
// Panel p = columns [k0, k1), next panel [k1, k2), previous panel `prev` = [q0, k0).  What the chain of
// panel p needs is that its OWN columns hold every earlier panel's contribution; everything else may lag.
//   launch              chain part                         riders
//   D(p)   diag block 0 (+ K = 64 prologue: prev's last    PH3(prev): prev's last sub-block -> panel p's columns (not its
//          sub-block, if PH3 is pending)                   tile (0,0)); ROWS(prev); NEAR(prev) 1st part; FAR(prev) share
//   L1(p)  solve sub-block 0 | diag block 1                NEAR(prev) rest; FAR(prev) share
//   L2(p)  solve sub-block 1 | diag block 2                PH(p, 0): sub-block 0 of p -> panel p+1's columns (K = 64); FAR(prev)
//   L3(p)  solve sub-block 2 | diag block 3                PH(p, 1); FAR(prev) share
//   T(p)   solve sub-block 3                               PH(p, 2); FAR(prev) rest
// with  NEAR(prev) = panel p+1's columns (all rows from k1) -= prev's panel, K = 256
//       FAR(prev)  = lower triangle from k2 on             -= prev's panel, K = 256
//       ROWS(prev) = carried rows, columns from k0 on      -= their own prev columns x prev's panel.
// Who writes what when: panel p's columns -- PH3(prev) in D(p) only, beside workgroup 0 on a different tile;
// panel p+1's columns -- NEAR(prev) in D, L1, then PH(p, s) from L2 on; beyond -- FAR(prev) only; launches of
// one queue follow one another, so each of these sets is complete before its first reader starts.
// `prev_w` > 0: the sweep starts behind a final panel [k_begin - prev_w, k_begin) whose contribution has been
// applied to panel k_begin's columns ONLY (the tail of a look-ahead factorisation, after its last head update).
// ---------------------------------------------------------------------------
// Optional second queue of a fused sweep: while FAR(prev) is large the riders cannot hide it (the first panels of
// a tail were rider-bound: 225 us per panel at 4352 trailing rows against a chain of ~115), so it runs as a
// persistent launch on `bulk` within `cus` compute units, beside the chain on the others.  FAR(prev) touches
// columns from k2 on only, the chain of panel p and its riders (PH3, NEAR, PH) the columns before k2: nothing
// else to order than "FAR of the panel before last is done" before a chain starts and "prev is final" before a FAR.
struct FarBulk {
    hipStream_t bulk = nullptr;
    std::vector<hipEvent_t>* ev = nullptr;
    size_t* ne = nullptr;
    int cus = 0;
    int64_t min_rows = 1 << 30;          // FAR on the bulk queue while n - k2 >= min_rows
    // called once per panel [k0, k1) after its chain has been enqueued, with an event that says "panel final"
    // (carried rows that follow the factorisation on queues of their own)
    std::function<int(int64_t, int64_t, hipEvent_t)> on_final;
};

template <typename T>
static int fused_sweep(T* kmat, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb,
                       PotrfBatch bt, hipStream_t st, int64_t k_begin = 0, int64_t prev_w = 0, const FarBulk* fb = nullptr)
{
    const char* fn = "cimrgp_potrf";
    const bool rows = (b != nullptr && m > 0);
    hipEvent_t ev_prev_final = nullptr;                     // (far-bulk mode) panel `prev` is final, on st
    hipEvent_t ev_far_last = nullptr;                       // (far-bulk mode) the last FAR launched on the bulk queue
    auto next_event = [&]() { return (*fb->ev)[(*fb->ne)++]; };
    if (fb && prev_w > 0) {
        ev_prev_final = next_event();
        hipError_t e = hipEventRecord(ev_prev_final, st);
        if (e != hipSuccess) return check_hip(e, fn, "hipEventRecord");
    }
    // the chain parts of the five launches last about this long alone (us; round 4, as measured in the tail of an
    // N = 8192 factorisation without riders' help)
    static const double chain_us[5] = {15.0, 21.0, 24.0, 28.0, 13.0};
    int64_t q0 = (prev_w > 0) ? k_begin - prev_w : -1;      // previous panel (-1: none)
    int64_t qw = prev_w;
    bool ph3_pending = false;                                // prev's last sub-block still owed to this panel's columns
    bool rows_pending = false;                               // ROWS(prev) owed (at a tail entry the rows have seen prev already)
    auto tiles64 = [](int64_t v) { return (v + 63) / 64; };
    for (int64_t k0 = k_begin; k0 < n; k0 += CIMRGP_NB) {
        const int64_t w = (n - k0 < CIMRGP_NB) ? (n - k0) : CIMRGP_NB;
        const int64_t k1 = k0 + w;
        const int64_t wn = (k1 < n) ? ((n - k1 < CIMRGP_NB) ? (n - k1) : CIMRGP_NB) : 0;
        const int64_t k2 = k1 + wn;
        Riders<T> rd[5];
        for (int i = 0; i < 5; ++i) rd[i] = no_riders<T>();
        bool far_launched = false;
        auto add = [&](int launch, const RiderJob<T>& jb) {
            if (jb.count <= 0) return;
            Riders<T>& r = rd[launch];
            r.job[r.njobs++] = jb;
            r.total += jb.count;
        };
        auto rect_job = [&](T* c, int64_t ldc, const T* a, int64_t lda, const T* bb, int64_t ldbb, int64_t mm, int64_t nn, int64_t kk) {
            RiderJob<T> jb;
            jb.c = c; jb.a = a; jb.b = bb; jb.ldc = ldc; jb.lda = lda; jb.ldb = ldbb;
            jb.m = (int)mm; jb.n = (int)nn; jb.k = (int)kk; jb.lower = 0; jb.tiles_n = (int)tiles64(nn);
            jb.first = 0; jb.count = (int)(tiles64(mm) * tiles64(nn)); jb.skip00 = 0; jb.rows_job = 0;
            return jb;
        };
        if (q0 >= 0) {
            const T* pa = kmat + q0;                          // prev's panel columns, row r at pa + r * ld
            if (ph3_pending) {
                // prev's last 64 columns -> this panel's columns, every row from k0 (tile (0,0) is workgroup 0's)
                RiderJob<T> jb = rect_job(kmat + k0 * ld + k0, ld, kmat + k0 * ld + (k0 - SB), ld, kmat + k0 * ld + (k0 - SB), ld,
                                          n - k0, w, SB);
                jb.skip00 = 1;
                add(0, jb);
            }
            int64_t ph3_tiles = rd[0].total;                  // K = 64 tiles
            int64_t rows_near_tiles = 0, rows_far_tiles = 0;
            if (rows_pending) {
                // the carried rows' columns of THIS panel: needed by the panel's first link (which solves them)
                RiderJob<T> jb = rect_job(b + k0, ldb, b + q0, ldb, pa + k0 * ld, ld, m, w, qw);
                jb.rows_job = 1;
                add(0, jb);
                rows_near_tiles = jb.count;
                if (wn > 0) rows_far_tiles = tiles64(m) * tiles64(n - k1);      // ... and everything right of it: any launch
            }
            if (wn > 0) {
                const int64_t near_tiles = tiles64(n - k1) * tiles64(wn);
                const int64_t tf = (n > k2) ? tiles64(n - k2) : 0;
                // FAR(prev) on the bulk queue (persistent, fb->cus units) while it is large; as riders otherwise
                const bool far_on_bulk = fb && fb->cus >= 8 && ev_prev_final && bt.count == 1 && n - k2 >= fb->min_rows && (n - k2) % 128 == 0 &&
                                         qw == CIMRGP_NB && gemm_pers_head_tiles(n - k2, (int)qw, (int)sizeof(T)) > 0;
                if (far_on_bulk) {
                    hipError_t e = hipStreamWaitEvent(fb->bulk, ev_prev_final, 0);
                    if (e != hipSuccess) return check_hip(e, fn, "hipStreamWaitEvent");
                    GemmBatch gb; gb.pers = fb->cus; gb.pers_force = 1;
                    const double mm = (double)(n - k2);
                    hipEvent_t rec = rec_open(fb->bulk, mm * (mm + 1.0) * (double)qw, (mm * (mm + 1.0) + mm * (double)qw) * (double)sizeof(T));
                    int rcf = gemm_nt_sub<T>(kmat + k2 * ld + k2, ld, pa + k2 * ld, ld, pa + k2 * ld, ld, n - k2, n - k2, (int)qw, true, fb->bulk, gb);
                    if (rec) (void)hipEventRecord(rec, fb->bulk);
                    if (rcf) return rcf;
                    far_launched = true;
                }
                const int64_t far_tiles = far_on_bulk ? 0 : tf * (tf + 1) / 2;
                // How many of these K = 256 tiles each launch takes.  A launch's riders run in ROUNDS of
                // (2 workgroups per compute unit - the launch's own chain workgroups), ~20 us per round of
                // K = 256 tiles, and a launch lasts max(its chain part, its rounds): whole rounds are given
                // to the launches whose chain part they lengthen least (a launch with 1.3 rounds of riders
                // takes two rounds' time: the first version of this schedule, split by the chain parts'
                // durations, took 221 us per panel at 4352 trailing rows where 7 packed rounds take ~150).
                const int slots = 2 * (far_on_bulk ? 256 - fb->cus : 256);
                const double t_round = (double)knobs().rider_round_us;
                const int64_t rows_below = n - k1;
                int nchain_i[5], fixed_i[5];
                for (int i = 0; i < 5; ++i) {
                    // rows the launch's panel solve covers: below diagonal block i + 1 (links), below the panel (last solve)
                    const int64_t below = (i == 4) ? rows_below : n - k0 - SB * (i + 1);
                    nchain_i[i] = (i == 0) ? 1 : (int)((below + TR - 1) / TR) + (i < 4 ? 1 : 0) + (int)(((rows ? m : 0) + TR - 1) / TR);
                    fixed_i[i] = 0;
                }
                // riders already placed (PH3, ROWS in launch 0; this panel's PH(p, s) go to launches 2..4: K = 64 tiles,
                // about a third of a K = 256 tile each)
                fixed_i[0] = (int)(ph3_tiles / 3 + rows_near_tiles);
                if (w == CIMRGP_NB) for (int i = 2; i < 5; ++i) fixed_i[i] = (int)(tiles64(n - k1) * tiles64(wn)) / 3;
                // Round 4: a launch starts with NO round of K = 256 riders; rounds go first to the launches whose
                // chain part outlasts a round anyway (the links), and the first diagonal kernel and the last solve --
                // 15 and 13 us alone, 25-29 and 16 with a round of riders -- take riders only when the links are full
                // (HISTORY.md, round 4).
                int rounds[5] = {0, 0, 0, 0, 0};
                auto capacity = [&](int i) { const int64_t c = (int64_t)rounds[i] * (slots - nchain_i[i]) - fixed_i[i]; return c > 0 ? c : 0; };
                const int64_t need = near_tiles + far_tiles + rows_far_tiles;
                for (;;) {
                    int64_t cap = 0;
                    for (int i = 0; i < 5; ++i) cap += capacity(i);
                    // NEAR must fit launches 0 and 1
                    const bool near_ok = capacity(0) + capacity(1) >= near_tiles;
                    if (cap >= need && near_ok) break;
                    int best = -1;
                    double best_cost = 1e30;
                    for (int i = (near_ok ? 0 : 0); i < (near_ok ? 5 : 2); ++i) {
                        const double now = (rounds[i] * t_round > chain_us[i]) ? rounds[i] * t_round : chain_us[i];
                        const double then = ((rounds[i] + 1) * t_round > chain_us[i]) ? (rounds[i] + 1) * t_round : chain_us[i];
                        const double cost = (then - now) / (double)(slots - nchain_i[i]);
                        if (cost < best_cost - 1e-12) { best_cost = cost; best = i; }
                    }
                    ++rounds[best];
                    if (rounds[best] > 64) break;           // cannot happen (guards the loop)
                }
                // NEAR(prev): launches 0 and 1 only (from launch 2 on this panel's sub-blocks update the same columns)
                RiderJob<T> nr = rect_job(kmat + k1 * ld + k1, ld, pa + k1 * ld, ld, pa + k1 * ld, ld, n - k1, wn, qw);
                int64_t near0 = 0;                                                           // the first link before the diagonal kernel
                if (near_tiles - near0 > capacity(1)) near0 = near_tiles - capacity(1);     // (capacities cover it: near_ok)
                RiderJob<T> n0 = nr; n0.first = 0; n0.count = (int)near0; add(0, n0);
                RiderJob<T> n1 = nr; n1.first = (int)near0; n1.count = (int)(near_tiles - near0); add(1, n1);
                {
                    // FAR(prev), then the carried rows' far update, over the launches' remaining capacities
                    RiderJob<T> fr;
                    fr.c = kmat + k2 * ld + k2; fr.a = pa + k2 * ld; fr.b = pa + k2 * ld; fr.ldc = fr.lda = fr.ldb = ld;
                    fr.m = fr.n = (int)(n - k2); fr.k = (int)qw; fr.lower = 1; fr.tiles_n = (int)tf; fr.skip00 = 0; fr.rows_job = 0;
                    fr.first = 0; fr.count = 0;
                    RiderJob<T> rf = fr;
                    if (rows_far_tiles > 0) {
                        rf = rect_job(b + k1, ldb, b + q0, ldb, pa + k1 * ld, ld, m, n - k1, qw);
                        rf.rows_job = 1;
                    }
                    int64_t done_f = 0, done_r = 0;
                    static const int order[5] = {1, 2, 3, 0, 4};
                    for (int oi = 0; oi < 5; ++oi) {
                        const int i = order[oi];
                        int64_t room = capacity(i) - (i == 0 ? near0 : i == 1 ? (near_tiles - near0) : 0);
                        if (room < 0) room = 0;
                        int64_t take_f = far_tiles - done_f;
                        if (oi < 4 && take_f > room) take_f = room;
                        room -= take_f;
                        int64_t take_r = rows_far_tiles - done_r;
                        if (oi < 4 && take_r > room) take_r = (room > 0 ? room : 0);
                        if (take_f > 0) { RiderJob<T> part = fr; part.first = (int)done_f; part.count = (int)take_f; add(i, part); }
                        if (take_r > 0) { RiderJob<T> part = rf; part.first = (int)done_r; part.count = (int)take_r; add(i, part); }
                        done_f += take_f;
                        done_r += take_r;
                    }
                }
            }
        }
        if (wn > 0 && w == CIMRGP_NB) {
            // this panel's sub-blocks 0, 1, 2 -> the next panel's columns, each as soon as it is final
            for (int sblk = 0; sblk < 3; ++sblk) {
                const int64_t cs = k0 + SB * sblk;
                add(2 + sblk, rect_job(kmat + k1 * ld + k1, ld, kmat + k1 * ld + cs, ld, kmat + k1 * ld + cs, ld, n - k1, wn, SB));
            }
        }
        if (fb) {
            // the FAR launched during the previous iteration wrote the columns this chain's riders (and, when FAR
            // rides again, its FAR tiles) are about to touch
            if (ev_far_last) {
                hipError_t e = hipStreamWaitEvent(st, ev_far_last, 0);
                if (e != hipSuccess) return check_hip(e, fn, "hipStreamWaitEvent");
                ev_far_last = nullptr;
            }
            if (far_launched) {
                ev_far_last = next_event();
                hipError_t e = hipEventRecord(ev_far_last, fb->bulk);
                if (e != hipSuccess) return check_hip(e, fn, "hipEventRecord");
            }
        }
        int rc = panel_chain<T>(kmat, n, ld, ws, info, k0, w, b, m, ldb, bt, st, fn, true, false, rd, ph3_pending);
        if (rc) return rc;
        if (fb && (k1 < n || fb->on_final)) {
            ev_prev_final = next_event();
            hipError_t e = hipEventRecord(ev_prev_final, st);
            if (e != hipSuccess) return check_hip(e, fn, "hipEventRecord");
            if (fb->on_final) {
                rc = fb->on_final(k0, k1, ev_prev_final);
                if (rc) return rc;
            }
        }
        q0 = k0;
        qw = w;
        ph3_pending = (wn > 0 && w == CIMRGP_NB);
        rows_pending = rows && k1 < n;
        // a ragged panel that still has columns to its right cannot happen (only the last panel is ragged)
    }
    if (fb && ev_far_last) {
        hipError_t e = hipStreamWaitEvent(st, ev_far_last, 0);
        if (e != hipSuccess) return check_hip(e, fn, "hipStreamWaitEvent");
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Factorisation with one-panel look-ahead.  The trailing update of panel p is
// split into the columns of panel p+1 ("head", rectangular) and the rest (lower
// SYRK).  As soon as the head is done, panel p+1 is factored on a second,
// high-priority stream while the main stream is still busy with the rest; the
// latency-bound panel chain (64 sequential columns per diagonal block) hides
// behind the MFMA-bound update for as long as the trailing matrix is large.
// Fork/join by events only (graph-capturable); the side stream and the event
// pool are created once per device and reused.
// ---------------------------------------------------------------------------
namespace {
constexpr int MAX_CTX = 8;               // look-ahead contexts per device: one per concurrently factoring caller stream
constexpr int64_t SINGLE_QUEUE_MAX = 5120;   // n at or below this: one queue, no look-ahead (see potrf_run)

struct LookAhead {
    hipStream_t side = nullptr;        // panel chain (high priority, all compute units)
    hipStream_t bulk = nullptr;        // trailing updates (unused: the caller's stream runs them)
    hipStream_t rows = nullptr;        // carried rows: lags behind the factorisation
    hipStream_t rows_far = nullptr;    // carried rows: far part of each panel's update (beside the rows' own panel chain)
    std::vector<hipEvent_t> ev;
    int* flag = nullptr;               // device counter: head tiles stored by the combined update launches (k_gate polls it)
    hipStream_t owner = nullptr;       // the caller stream this context was created for
    bool gate_ok = false;              // this context may hold a kernel that waits for another one (k_gate): the device's first context only
    std::mutex enqueue;                // one factorisation at a time enqueues on this context's queues
    hipEvent_t last_done = nullptr;    // behind the latest look-ahead factorisation on this context (recorded on its caller's stream)
};
std::mutex g_reg_mutex;                // guards g_ctx and context creation
std::vector<LookAhead*> g_ctx[16];     // per device; contexts live as long as the process

// Streams of one context.  All three or none: a context without its rows queue would have to
// order the carried rows on the caller's stream, which the schedule below does not do.
LookAhead* make_ctx(int dev)
{
    LookAhead* la = new LookAhead;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    bool ok = hipStreamCreateWithPriority(&la->side, hipStreamNonBlocking, hi) == hipSuccess;
    // (Round 2 could run the update kernels on CU-masked queues -- hipExtStreamCreateWithCUMask,
    // CIMRGP_RESERVE_CUS -- to keep compute units free for the chain: measured useless three times
    // (HISTORY.md, rounds 1-2, rejected (i)) and removed in round 3: masked streams are BLOCKING streams that
    // synchronise with the legacy default stream, and they were the one kind of object still alive at
    // process exit in the profiler runs that crashed in an exit handler.  The persistent update kernel
    // splits the machine instead: a launch of G workgroups occupies G compute units.)
    if (ok) ok = hipStreamCreateWithPriority(&la->rows, hipStreamNonBlocking, lo) == hipSuccess;
    if (ok) ok = hipMalloc(&la->flag, 256) == hipSuccess;
    // (the carried rows' second queue is created on first use: ensure_rows_far)
    if (!ok) {
        if (la->side) (void)hipStreamDestroy(la->side);
        if (la->bulk) (void)hipStreamDestroy(la->bulk);
        if (la->rows) (void)hipStreamDestroy(la->rows);
        if (la->rows_far) (void)hipStreamDestroy(la->rows_far);
        if (la->flag) (void)hipFree(la->flag);
        delete la;
        return nullptr;
    }
    return la;
}

// The context serving caller stream `st` on the current device (created on first use under the
// registry lock; beyond MAX_CTX contexts callers share one by stream hash, which only serialises
// them on its queues).  Independent blocks of a layer are factored on different caller streams
// and so get different contexts: their panel chains run side by side.
LookAhead* acquire_ctx(hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    std::lock_guard<std::mutex> guard(g_reg_mutex);
    std::vector<LookAhead*>& list = g_ctx[dev];
    for (LookAhead* la : list)
        if (la->owner == st) return la;
    if ((int)list.size() < MAX_CTX) {
        LookAhead* la = make_ctx(dev);
        if (la == nullptr) return list.empty() ? nullptr : list[0];
        la->owner = st;
        // One context per device may use the gate.  Streams share the runtime's four hardware queues; with two
        // gate users a gate of A could sit in front of the update B's gate waits for and vice versa.  Within one
        // context the update is always enqueued ahead of its gate, so a single user cannot block itself.
        la->gate_ok = list.empty();
        list.push_back(la);
        return la;
    }
    return list[(reinterpret_cast<uintptr_t>(st) >> 6) % MAX_CTX];
}

// Destroys every look-ahead context (streams, events) of every device.  The caller guarantees that no
// factorisation is in flight or will be enqueued concurrently (cimrgp_shutdown).
int destroy_contexts()
{
    std::lock_guard<std::mutex> guard(g_reg_mutex);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (int dev = 0; dev < 16; ++dev) {
        if (g_ctx[dev].empty()) continue;
        (void)hipSetDevice(dev);
        for (LookAhead* la : g_ctx[dev]) {
            for (hipStream_t q : {la->side, la->bulk, la->rows, la->rows_far})
                if (q) { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); }
            for (hipEvent_t e : la->ev) (void)hipEventDestroy(e);
            if (la->last_done) (void)hipEventDestroy(la->last_done);
            if (la->flag) (void)hipFree(la->flag);
            delete la;
        }
        g_ctx[dev].clear();
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return 0;
}

// Event pool of a context; call with la->enqueue held.
bool grow_events(LookAhead* la, size_t nevents)
{
    while (la->ev.size() < nevents) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
        la->ev.push_back(e);
    }
    return true;
}

template <typename T>
int factor_panel(T* kmat, int64_t n, int64_t ld, T* ws, int32_t* info, int64_t k0, int64_t w, hipStream_t st, bool alone,
                 bool first_done = false)
{
    return panel_chain<T>(kmat, n, ld, ws, info, k0, w, (T*)nullptr, 0, 0, PotrfBatch(), st, "cimrgp_potrf", alone, first_done);
}
}  // namespace

// The queue of `st`'s look-ahead context that is idle between two factorisations on `st` (the carried rows' own
// queue: the rows of a factorisation start ~2 ms after its first panel at N = 8192): a caller that pipelines independent
// blocks runs the latency-bound solve / prediction of block i there, beside the first panels of block i+1
// (cimrgp_solve_queue).  A fifth stream of the caller's own for that purpose costs more than it hides (measured: 8.1 ->
// 10.2 ms per step; the runtime serves four hardware queues).  `st` itself when it owns no context.
hipStream_t solve_queue_for(hipStream_t st)
{
    LookAhead* la = acquire_ctx(st);
    return (la != nullptr && la->owner == st && la->rows != nullptr) ? la->rows : st;
}


// The queue of `st`'s look-ahead context that falls idle BEFORE a factorisation on `st` ends (the panel chain's queue: the
// last third of a factorisation runs on one queue, potrf_run's tail): the front end of the NEXT independent block can run
// there beside that tail (cimrgp_front_queue).  `st` itself when it owns no context.
hipStream_t front_queue_for(hipStream_t st)
{
    LookAhead* la = acquire_ctx(st);
    return (la != nullptr && la->owner == st && la->side != nullptr) ? la->side : st;
}

int potrf_shutdown()
{
    {
        std::lock_guard<std::mutex> guard(g_profile_mutex);
        for (auto& r : g_recs) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
        for (auto& r : g_free) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
        g_recs.clear();
        g_free.clear();
        g_profile = false;
    }
    return destroy_contexts();
}

// Workspace layout: [ceil(n/64) slabs of 64x64 inverses][ceil(n/256) blocks of 256x256 invT].
template <typename T>
static int build_invT(const T* kmat, int64_t n, int64_t ld, T* ws, hipStream_t st, PotrfBatch bt = PotrfBatch())
{
    const char* fn = "cimrgp_potrf";
    const int64_t nslab = (n + SB - 1) / SB, npan = (n + CIMRGP_NB - 1) / CIMRGP_NB;
    T* invT = ws + nslab * (SB * SB);
    const unsigned nbatch = (unsigned)bt.count;
    // Full panels (round 4): invT_p = I L_pp^-T is the carried rows' panel step applied to the identity -- one launch of
    // k_rows_step for all of them (16 workgroups per panel, ~12 us) instead of k_invT_panel's four dependent sub-steps
    // per 32-row strip with their global round trips (40 us at the end of every factorisation); a ragged last panel
    // keeps k_invT_panel.
    // (single matrices only: in a batch of many small blocks the 16-row workgroups' traffic on the diagonal blocks costs
    // more than the strips' latency -- 128 blocks of 2048: fit 11.6 -> 12.2 ms)
    const int64_t nfull = (bt.count == 1) ? n / CIMRGP_NB : 0;
    const int64_t blk = (int64_t)CIMRGP_NB * CIMRGP_NB;
    if (nfull > 0) {
        hipLaunchKernelGGL((k_rows_step<T, false>), dim3(CIMRGP_NB / RowsStep<T>::R, (unsigned)(nfull * bt.count)), dim3(256), 0, st,
                           invT, (int64_t)CIMRGP_NB, (int)CIMRGP_NB, kmat, ld, (const T*)ws, (const T*)nullptr, (int64_t)0, 2, (int)nfull,
                           blk, CIMRGP_NB * ld + CIMRGP_NB, (int64_t)(CIMRGP_NB / SB) * (SB * SB), (int64_t)0,
                           bt.sws, bt.sk, bt.sws);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    if (npan > nfull) {
        hipLaunchKernelGGL((k_invT_panel<T>), dim3(CIMRGP_NB / TR, (unsigned)(npan - nfull), nbatch), dim3(256), 0, st,
                           invT, kmat, ld, (int)n, (const T*)ws, bt.sk, bt.sws, (int)nfull);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    // Round 4: the backward solve takes TWO panels per step through the 512 x 512 inverse
    //     [A 0; B C]^-T = [A^-T  X; 0  C^-T],   X = -A^-T B^T C^-T  (256 x 256, dense),
    // halving its chain of dependent launches (62 -> 32 at n = 8192: 0.33 -> 0.2 ms).  X is what the carried rows' panel
    // step computes for the rows of A^-T (already there: invT of the pair's first panel) with a zero right-hand side:
    // one launch of k_rows_step for all pairs of full panels, behind the inverses (potrs_run: bwd_pairs).
    // Above the one-queue size only (bwd_pairs(n) in common.hpp: the solve applies the same rule): below it the launch that
    // builds X costs what the shorter chain saves.
    const int64_t npairs = bwd_pairs(n);
    if (npairs > 0) {
        T* xbase = invT + npan * (CIMRGP_NB * CIMRGP_NB);
        hipLaunchKernelGGL((k_rows_step<T, true>), dim3(CIMRGP_NB / RowsStep<T>::R, (unsigned)(npairs * bt.count)), dim3(256), 0, st,
                           xbase, (int64_t)CIMRGP_NB, (int)CIMRGP_NB, (const T*)(kmat + (int64_t)CIMRGP_NB * ld), ld,
                           (const T*)(ws + (CIMRGP_NB / SB) * (SB * SB)), (const T*)invT, (int64_t)CIMRGP_NB, 1, (int)npairs,
                           blk, 2 * CIMRGP_NB * ld + 2 * CIMRGP_NB, (int64_t)(2 * CIMRGP_NB / SB) * (SB * SB), 2 * blk,
                           bt.sws, bt.sk, bt.sws);
        CIMRGP_LAUNCH_CHECK(fn);
    }
    return 0;
}

#define CIMRGP_HIP_TRY(call, what) \
    do { hipError_t e__ = (call); if (e__ != hipSuccess) return check_hip(e__, "cimrgp_potrf", what); } while (0)

template <typename T>
int potrf_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb, hipStream_t st, hipStream_t ready_on)
{
    const bool rows = (b != nullptr && m > 0);
    const int64_t npanels = (n + CIMRGP_NB - 1) / CIMRGP_NB;
    // Small matrices: one queue.  Measured in round 1 (whole potrf, one queue vs look-ahead): n = 2048:
    // 1.23 vs 1.37 ms, 4096: 2.80 vs 3.04 -- and independent blocks of a layer run concurrently on
    // their callers' streams, which fills the machine better than look-ahead inside each of them.
    LookAhead* la = (n > SINGLE_QUEUE_MAX && npanels > 2) ? acquire_ctx(st) : nullptr;
    // `ready_on`: the queue on which the caller wrote K and B, when that is this context's chain queue (cimrgp_front_queue) and
    // not `st`.  The FIRST panel's chain then follows them there in queue order instead of waiting for `st` -- for a caller that
    // pipelines independent blocks it runs beside the previous factorisation's latency-bound tail, not behind it (~100 us of a
    // nearly idle machine per factorisation).  Everything after it waits for `st` as before.
    const bool early = la != nullptr && ready_on != nullptr && ready_on == la->side && ready_on != st;
    CIMRGP_HIP_TRY(hipMemsetAsync(info, 0, sizeof(int32_t), early ? la->side : st), "hipMemsetAsync(info)");
    if (la == nullptr) {
        int rc0 = fused_sweep<T>(k, n, ld, ws, info, b, m, ldb, PotrfBatch(), st);
        return rc0 ? rc0 : build_invT<T>(k, n, ld, ws, st);
    }

    // Host threads whose streams share a context serialise their ENQUEUE (microseconds); distinct
    // caller streams have distinct contexts and enqueue concurrently.
    std::lock_guard<std::mutex> guard(la->enqueue);
    if (!grow_events(la, (size_t)(9 * npanels + 16 + 4))) return fail("cimrgp_potrf", "hipEventCreate failed");
    hipStream_t sp = la->side;
    hipStream_t sb = la->bulk ? la->bulk : st;         // bulk trailing updates
    size_t ne = 0;
    // The device counter of the gate belongs to the CONTEXT, and beyond MAX_CTX contexts a context serves caller
    // streams other than its owner (acquire_ctx, by hash).  Only the owner's factorisations may reset and count on
    // it: a second caller stream would reset the counter under the owner's in-flight gates (which then expire) and
    // have its own gates satisfied by the owner's tiles (a silently wrong factor).  Everybody else keeps the head
    // update on the chain queue (round 2's schedule), which needs no counter.
    const bool may_gate = la->gate_ok && la->owner == st;
    // Everything below enqueues on several queues; an error return in the middle must not leave the caller's
    // stream running ahead of work already queued on them (the caller may free or reuse K / workspace / B):
    // the enqueue proper is `body`, and whatever it returns the queues are joined into `st` behind it.
    auto body = [&]() -> int {
    // The side stream runs the whole latency-bound chain in stream order -- "head" update of the
    // next panel's columns, then that panel's factorisation -- so that no inter-queue signal
    // sits between two links of the chain; the caller's stream runs the bulk of each trailing
    // update (and, off the chain, the carried rows).  Cross-stream edges: "panel final"
    // (side -> main, before the bulk update that reads it) and "bulk update done" (main -> side,
    // before the next head touches columns the bulk update wrote).
    if (may_gate) CIMRGP_HIP_TRY(hipMemsetAsync(la->flag, 0, 256, st), "hipMemsetAsync(flag)");
    int flag_expected = 0;                             // head tiles the chain has been told to wait for so far
    hipEvent_t ev_start = la->ev[ne++];
    CIMRGP_HIP_TRY(hipEventRecord(ev_start, st), "hipEventRecord");
    if (!early) CIMRGP_HIP_TRY(hipStreamWaitEvent(sp, ev_start, 0), "hipStreamWaitEvent");
    if (sb != st) CIMRGP_HIP_TRY(hipStreamWaitEvent(sb, ev_start, 0), "hipStreamWaitEvent");
    int rc = factor_panel<T>(k, n, ld, ws, info, 0, (n < CIMRGP_NB) ? n : CIMRGP_NB, sp, true);
    if (rc) return rc;
    hipEvent_t ev_panel = la->ev[ne++];
    CIMRGP_HIP_TRY(hipEventRecord(ev_panel, sp), "hipEventRecord");
    hipEvent_t ev_rest = nullptr;                      // bulk update of the previous panel
    PanelGroup grp;                                    // open group of panels whose far update is still owed
    auto grp_open = [&]() { return grp.g0 >= 0; };
    bool tail_done = false;
    const int64_t single_tail_below = knobs().tail_below;
    hipEvent_t ev_bulk_last = nullptr;                 // last thing queued on the bulk stream
    // Bulk updates beside the chain: the persistent update kernel on all compute units but `chain_cus`,
    // which stay free for the chain's kernels (one persistent workgroup fills a unit's registers, so the
    // grid size IS the split).
    GemmBatch bulk_gb;
    if (knobs().gemm_pers > 0 && knobs().chain_cus > 0 && knobs().chain_cus < knobs().gemm_pers)
        bulk_gb.pers = knobs().gemm_pers - knobs().chain_cus;
    int64_t rows_next = 0;                             // first panel the carried rows have not seen yet
    // Panel k0 is final (event ev_final): solve + update the carried rows.  They form their own
    // chain (panel p+1 of the rows needs panel p of the rows) that depends on the factorisation
    // only through "panel k0 final", so it runs on its own queues and lags behind: nothing of it is
    // issued while the trailing updates are still large (that phase is MFMA-bound and the rows
    // would only take compute units away from the critical path); from then on it fills the
    // compute units the latency-bound panel chain leaves idle.
    // (Measured and rejected in round 2: cutting the rows into 2..4 slices on queues of their own so
    // that their latency-bound chains overlap -- 9.5 -> 10.1 / 12.6 / 21 ms at N = 8192 with 2050 rows:
    // more low-priority queues only add contention for the panel chain; 64-tile updates for the rows,
    // whose workgroups retire four times as often: 94.8 -> 92.6 posteriors/s; an earlier or later
    // start than 4608 trailing rows: 3072 / 5632 / 6656 / 8192 -> 89.2 / 94.3 / 91.6 / 89.5.)
    PanelGroup rows_grp;                               // carried rows: open group of panels whose far update is owed
    hipEvent_t ev_rows_far = nullptr;                  // carried rows: last far update queued on the second rows queue
    hipEvent_t ev_rows_far_prev = nullptr;             // ... and the one before it
    // second rows queue: created when first wanted (cimrgp_set_rows_queues(1) before the first
    // factorisation with carried rows means it never exists: a process then holds four streams)
    if (rows && rows_queues() == 2 && la->rows_far == nullptr) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&la->rows_far, hipStreamNonBlocking, lo) != hipSuccess) la->rows_far = nullptr;
    }
    const bool rows_pipeline = (rows_queues() == 2) && la->rows_far != nullptr;
    // trailing columns below which the carried rows start (set again below when this factorisation starts with early panels:
    // beside the previous factorisation's last panels the rows do better starting two panels later)
    int64_t rows_start = knobs().rows_start_below;
    auto rows_after_panel = [&](int64_t k0, int64_t k1, hipEvent_t ev_final) -> int {
        if (!rows) return 0;
        hipStream_t sq = la->rows;                     // always present (make_ctx: all queues or no context)
        if (n - k1 > rows_start && k1 < n) return 0;
        CIMRGP_HIP_TRY(hipStreamWaitEvent(sq, ev_final, 0), "hipStreamWaitEvent");
        // (pairing the rows' updates below that size was measured neutral-to-worse at N = 8192)
        for (int64_t r0 = rows_next; r0 <= k0; r0 += CIMRGP_NB) {
            const int64_t rw = (n - r0 < CIMRGP_NB) ? (n - r0) : CIMRGP_NB;
            const int64_t r1 = r0 + rw;
            const int64_t rn = (n - r1 < CIMRGP_NB) ? (n - r1) : CIMRGP_NB;
            if (!rows_pipeline || rows_grp.g0 >= 0 || (n > r1 + rn && group_size(n - (r1 + rn), knobs().rows_pair_above) > 1)) {
                // grouped far updates (large matrices): the rows' chain as one queue
                if (ev_rows_far) { CIMRGP_HIP_TRY(hipStreamWaitEvent(sq, ev_rows_far, 0), "hipStreamWaitEvent"); ev_rows_far = nullptr; }
                int rcr = rows_panel_step<T>(b, ldb, m, k, ld, n, ws, r0, rows_grp, knobs().rows_pair_above, sq, "cimrgp_potrf_rows");
                if (rcr) return rcr;
                continue;
            }
            // The rows' own chain on `sq`: panel r0's solve with the previous panel's update of its columns fused in
            // (k_rows_step; until round 4 a 64-tile update and k_trsm256, two latency-bound launches); the update of
            // everything beyond the next panel (the bulk of the flops) on a second queue.  far(p) needs the solved
            // columns of panel p only and writes the columns from panel p+2 on: the step of panel p+2 waits for it,
            // the step of panel p+1 does not.
            const bool near_pending = rows_grp.near_pending;
            rows_grp.near_pending = false;
            if (rw == CIMRGP_NB) {
                if (near_pending && ev_rows_far_prev) CIMRGP_HIP_TRY(hipStreamWaitEvent(sq, ev_rows_far_prev, 0), "hipStreamWaitEvent");
                int rcs = rows_step_launch<T>(b, ldb, m, k, ld, ws, r0, near_pending, sq, "cimrgp_potrf_rows");
                if (rcs) return rcs;
            } else {
                if (near_pending) {              // (a promise is made for full panels only)
                    if (ev_rows_far_prev) CIMRGP_HIP_TRY(hipStreamWaitEvent(sq, ev_rows_far_prev, 0), "hipStreamWaitEvent");
                    int rcn = gemm_nt_sub<T>(b + r0, ldb, b + r0 - CIMRGP_NB, ldb, k + r0 * ld + r0 - CIMRGP_NB, ld, m, rw, CIMRGP_NB, false, sq);
                    if (rcn) return rcn;
                }
                hipLaunchKernelGGL((k_trsm256<T>), dim3((unsigned)((m + TR - 1) / TR)), dim3(256), 0, sq,
                                   b + r0, ldb, (int)m, (int)rw, (const T*)(k + r0 * ld + r0), ld,
                                   (const T*)(ws + (r0 / SB) * (SB * SB)));
                CIMRGP_LAUNCH_CHECK("cimrgp_potrf_rows");
            }
            if (n <= r1) continue;
            hipEvent_t ev_w = la->ev[ne++];
            CIMRGP_HIP_TRY(hipEventRecord(ev_w, sq), "hipEventRecord");
            int rcr = 0;
            if (rw == CIMRGP_NB && rn == CIMRGP_NB) {
                rows_grp.near_pending = true;
            } else {
                if (ev_rows_far) CIMRGP_HIP_TRY(hipStreamWaitEvent(sq, ev_rows_far, 0), "hipStreamWaitEvent");
                rcr = gemm_nt_sub<T>(b + r1, ldb, b + r0, ldb, k + r1 * ld + r0, ld, m, rn, (int)rw, false, sq);
                if (rcr) return rcr;
            }
            ev_rows_far_prev = ev_rows_far;
            if (n > r1 + rn) {
                hipStream_t sf = la->rows_far;
                CIMRGP_HIP_TRY(hipStreamWaitEvent(sf, ev_w, 0), "hipStreamWaitEvent");
                // The far update: whole 128-row tiles of the rows on the persistent kernel within a budget of compute
                // units (it then cannot crowd the factorisation out of the machine the way a 1000-workgroup launch of
                // the tile-per-workgroup kernel does), the few rows left over (the q target rows) in a thin launch.
                const int64_t m128 = (knobs().rows_cus >= 8 && knobs().gemm_pers >= 8) ? (m / 128) * 128 : 0;
                const int64_t nfar = n - (r1 + rn);
                if (m128 >= 128 && nfar % 128 == 0 && (m128 / 128) * (nfar / 128) >= 2 * knobs().rows_cus) {
                    GemmBatch gb; gb.pers = knobs().rows_cus; gb.pers_force = 1;
                    rcr = gemm_nt_sub<T>(b + r1 + rn, ldb, b + r0, ldb, k + (r1 + rn) * ld + r0, ld, m128, nfar, (int)rw, false, sf, gb);
                    if (rcr) return rcr;
                    if (m > m128) {
                        // On the rows' CHAIN queue (round 4), not behind the persistent launch: the far updates of the
                        // 128-row tiles run back to back on `sf` and are the critical path of this phase; this thin
                        // launch (240 workgroups for 2 rows, 17-65 us when the units are busy, plus a queue gap)
                        // took a fifth of that queue's time.  The thin rows are independent of the others, and on `sq`
                        // the next panel's step -- their only reader -- follows in queue order.
                        GemmBatch g0; g0.pers = 0;
                        rcr = gemm_nt_sub<T>(b + m128 * ldb + r1 + rn, ldb, b + m128 * ldb + r0, ldb, k + (r1 + rn) * ld + r0, ld,
                                             m - m128, nfar, (int)rw, false, sq, g0);
                    }
                } else {
                    rcr = gemm_nt_sub<T>(b + r1 + rn, ldb, b + r0, ldb, k + (r1 + rn) * ld + r0, ld, m, nfar, (int)rw, false, sf);
                }
                if (rcr) return rcr;
                ev_rows_far = la->ev[ne++];
                CIMRGP_HIP_TRY(hipEventRecord(ev_rows_far, sf), "hipEventRecord");
            }
        }
        rows_next = k1;
        return 0;
    };
    int64_t k_begin = 0;
    if (early) {
        // ... and knobs().early_panels more panels one-queue style (update of everything right of panel p, then panel p+1, in
        // queue order on the chain queue): work of THIS factorisation done while the previous one's tail leaves the machine
        // two-thirds idle.  From panel k_begin on the look-ahead schedule below takes over, behind `st` as always.
        // (only while the context's previous factorisation is still in flight when this one is enqueued: with the machine
        //  to itself a factorisation is better off with look-ahead from the first panel on)
        const bool prev_in_flight = la->last_done != nullptr && hipEventQuery(la->last_done) == hipErrorNotReady;
        (void)hipGetLastError();                     // "not ready" is an answer, not an error for the launch checks below to find
        const int np_early = (sizeof(T) == 8 && prev_in_flight) ? knobs().early_panels : 0;
        GemmBatch early_gb = bulk_gb;
        if (knobs().early_cus >= 8) early_gb.pers = knobs().early_cus;
        for (int p = 0; p < np_early && rc == 0; ++p) {
            const int64_t k0e = (int64_t)p * CIMRGP_NB, k1e = k0e + CIMRGP_NB;
            if (n - k1e < 4 * CIMRGP_NB || (n - k1e) % 128 != 0) break;
            const double mme = (double)(n - k1e);
            hipEvent_t rec = rec_open(sp, mme * (mme + 1.0) * (double)CIMRGP_NB, (mme * (mme + 1.0) + mme * (double)CIMRGP_NB) * (double)sizeof(T));
            rc = gemm_nt_sub<T>(k + k1e * ld + k1e, ld, k + k1e * ld + k0e, ld, k + k1e * ld + k0e, ld, n - k1e, n - k1e, (int)CIMRGP_NB, true, sp, early_gb);
            if (rec) (void)hipEventRecord(rec, sp);
            if (rc) return rc;
            rc = factor_panel<T>(k, n, ld, ws, info, k1e, CIMRGP_NB, sp, true);
            if (rc) return rc;
            k_begin = k1e;
        }
        if (k_begin > 0) {
            rows_start = knobs().rows_start_below_early;
            ev_panel = la->ev[ne++];
            CIMRGP_HIP_TRY(hipEventRecord(ev_panel, sp), "hipEventRecord");
        }
        CIMRGP_HIP_TRY(hipStreamWaitEvent(sp, ev_start, 0), "hipStreamWaitEvent");
    }
    for (int64_t k0 = k_begin; k0 < n; k0 += CIMRGP_NB) {
        const int64_t w  = (n - k0 < CIMRGP_NB) ? (n - k0) : CIMRGP_NB;
        const int64_t k1 = k0 + w;
        // With carried rows (round 3): the last rows_beside_tail_below columns are factored by the same one-queue fused
        // sweep while the rows keep following on their own queues, one panel behind (the sweep tells them when a
        // panel is final).  Entered later than the tail without rows (2560 against 4864 trailing columns): while the
        // rows' far updates are large the sweep's riders would queue behind them for compute units (113 posteriors/s
        // entered at 4864 and 107 at 6144 against 117.3 without and 119.4 at 2560).
        const bool rows_beside = rows && knobs().rows_beside_tail_below > 0;
        if (k1 < n && !grp_open() && (rows_beside ? n - k1 <= knobs().rows_beside_tail_below
                                                  : (!rows && n - k1 <= single_tail_below))) {
            // ---- single-stream tail.  Once the trailing matrix is small the look-ahead no longer
            // pays: its chain kernels wait for slots beside the update and every panel costs an
            // inter-queue hop, while one queue runs 4 x (diag + solve) = 124 us plus ONE update of
            // everything right of the panel, all at full speed (measured whole potrf, single queue
            // vs look-ahead: n = 2048: 1.23 vs 1.37 ms, 4096: 2.80 vs 3.04, 6144: 4.84 vs 5.05,
            // 8192: 7.95 vs 7.73; hybrid at N = 8192: 7.86 -> 7.52 ms).  With carried rows the rows'
            // own queue fills the tail either way and the hybrid is neutral (9.69 vs 9.73 ms): not
            // used then.  Panel k0 is factored; the region right of it holds all earlier
            // panels' updates once the bulk queue has drained.
            CIMRGP_HIP_TRY(hipStreamWaitEvent(st, ev_panel, 0), "hipStreamWaitEvent");
            if (sb != st && ev_bulk_last) CIMRGP_HIP_TRY(hipStreamWaitEvent(st, ev_bulk_last, 0), "hipStreamWaitEvent");
            // Round 3: the tail is the fused one-queue sweep -- the head update of panel k0 (the next panel's
            // columns, all rows) in a launch of its own, everything after it rides in the chains' launches
            // (fused_sweep).  (Carried rows that caught up here and then rode along: HISTORY.md, round 3.)
            if (rows_beside) {
                // the carried rows keep following on their own queues (panel k0 here, the tail's panels from the sweep)
                rc = rows_after_panel(k0, k1, ev_panel);
                if (rc) return rc;
            }
            {
                const int64_t kn = k1 + ((n - k1 < CIMRGP_NB) ? (n - k1) : CIMRGP_NB);
                rc = gemm_nt_sub<T>(k + k1 * ld + k1, ld, k + k1 * ld + k0, ld, k + k1 * ld + k0, ld,
                                    n - k1, kn - k1, (int)w, false, st);
                if (rc) return rc;
                FarBulk fbk;
                fbk.bulk = sp;                              // the chain's queue of the look-ahead phase is free now
                fbk.ev = &la->ev;
                fbk.ne = &ne;
                fbk.cus = knobs().tail_far_cus;
                fbk.min_rows = knobs().tail_far_min_rows;
                if (rows_beside) {
                    fbk.cus = 0;                            // far updates as riders: the rows' far updates hold the persistent units
                    fbk.on_final = [&](int64_t f0, int64_t f1, hipEvent_t evf) { return rows_after_panel(f0, f1, evf); };
                }
                const bool use_fb = rows_beside || (!rows && fbk.cus >= 8 && knobs().gemm_pers >= 8);
                rc = fused_sweep<T>(k, n, ld, ws, info, (T*)nullptr, 0, 0, PotrfBatch(), st, k1, w, use_fb ? &fbk : nullptr);
                if (rc) return rc;
            }
            tail_done = true;
            break;
        }
        const hipEvent_t ev_final = ev_panel;          // panel k0 is final (recorded on the side stream)
        const int64_t wn = (k1 < n) ? ((n - k1 < CIMRGP_NB) ? (n - k1) : CIMRGP_NB) : 0;   // next panel
        const int64_t k2 = k1 + wn;
        // Round 3: head and bulk update of panel k0 as ONE persistent launch on the bulk queue.  Its first
        // tiles are the next panel's columns (the old "head": on the chain's queue it ran on the few compute
        // units the persistent bulk update leaves free -- 144 us for 1 Gflop at N = 8192, the longest link of
        // the chain); they are counted as they are stored and the chain waits for the count through a
        // one-workgroup gate kernel.  The next panel's first diagonal block does not wait: it takes its own
        // 64 x 64 update as its prologue (as before) and the rest of the first 128 x 128 tile along as riders.
        // (not while the carried rows are running: their kernels hold compute units the persistent workgroups
        // of the combined launch -- head tiles included -- would have to wait for: 114 -> 109 posteriors/s)
        // (measured again in round 5 with the rows on 192 units: 137.2 -> 135.4 / 134.3 posteriors/s, HISTORY.md)
        const bool rows_running = rows && (n - k1 <= rows_start);
        const int heads = (may_gate && !rows_running && w == CIMRGP_NB && wn == CIMRGP_NB && n > k2 && !grp_open() &&
                           group_size(n - k2 - ((n - k2 < CIMRGP_NB) ? (n - k2) : CIMRGP_NB), knobs().far_pair_above) == 1)
                              ? gemm_pers_head_tiles(n - k1, (int)w, (int)sizeof(T)) : 0;
        if (heads > 0) {
            // The persistent launch is ENQUEUED before the gate that waits for its head tiles: a tool that runs one
            // kernel at a time in submission order (rocprofv3 --pmc, HIP_LAUNCH_BLOCKING) then finds the count complete
            // when the gate runs, instead of running the gate first and timing it out.
            hipEvent_t ev_rest_prev = ev_rest;
            flag_expected += heads;
            // bulk queue: everything right of panel k0, the next panel's columns first, behind "panel k0 final" as an event.
            // (A device word posted by the chain and polled by a gate here: potrf n = 8192 5.43 -> 5.38 ms, the step
            // unchanged, and the gate sat out its watchdog under rocprofv3 --pmc -- round 5, HISTORY.md.)
            CIMRGP_HIP_TRY(hipStreamWaitEvent(sb, ev_final, 0), "hipStreamWaitEvent");
            const double mm = (double)(n - k1);
            hipEvent_t rec = rec_open(sb, mm * (mm + 1.0) * (double)w, (mm * (mm + 1.0) + mm * (double)w) * (double)sizeof(T));
            GemmBatch gb = bulk_gb;
            gb.head_first = 1;
            gb.flag = la->flag;
            rc = gemm_nt_sub<T>(k + k1 * ld + k1, ld, k + k1 * ld + k0, ld, k + k1 * ld + k0, ld, n - k1, n - k1, (int)w, true, sb, gb);
            if (rec) (void)hipEventRecord(rec, sb);
            if (rc) return rc;
            ev_rest = la->ev[ne++];
            CIMRGP_HIP_TRY(hipEventRecord(ev_rest, sb), "hipEventRecord");
            ev_bulk_last = ev_rest;
            // chain queue: first diagonal block (+ the rest of tile (0, 0) of 128 as riders), gate, the other links
            if (ev_rest_prev) CIMRGP_HIP_TRY(hipStreamWaitEvent(sp, ev_rest_prev, 0), "hipStreamWaitEvent");
            Riders<T> r0 = no_riders<T>();
            {
                RiderJob<T>& jb = r0.job[0];
                jb.c = k + k1 * ld + k1; jb.a = k + k1 * ld + k0; jb.b = k + k1 * ld + k0; jb.ldc = jb.lda = jb.ldb = ld;
                jb.m = 128; jb.n = 128; jb.k = (int)w; jb.lower = 0; jb.tiles_n = 2; jb.first = 0; jb.count = 4; jb.skip00 = 1; jb.rows_job = 0;
                r0.njobs = 1; r0.total = 4;
            }
            hipLaunchKernelGGL((k_diag64q<T>), dim3(1 + r0.total), dim3(Q_NT), 0, sp, k + k1 * ld + k1, ld, (int)SB,
                               (const T*)(k + k1 * ld + k0), (int)w, ws + (k1 / SB) * (SB * SB), info, (int)k1, (int64_t)0, (int64_t)0,
                               (int64_t)0, r0);
            CIMRGP_LAUNCH_CHECK("cimrgp_potrf");
            hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, sp, (const int*)la->flag, flag_expected, info);
            CIMRGP_LAUNCH_CHECK("cimrgp_potrf");
            rc = factor_panel<T>(k, n, ld, ws, info, k1, wn, sp, false, true);
            if (rc) return rc;
            hipEvent_t ev_next = la->ev[ne++];
            CIMRGP_HIP_TRY(hipEventRecord(ev_next, sp), "hipEventRecord");
            ev_panel = ev_next;
            rc = rows_after_panel(k0, k1, ev_final);
            if (rc) return rc;
            continue;
        }
        if (k1 < n) {
            // chain: head (columns of the next panel, all rows below), then the next panel
            if (ev_rest) CIMRGP_HIP_TRY(hipStreamWaitEvent(sp, ev_rest, 0), "hipStreamWaitEvent");
            // The next panel's FIRST diagonal block does not wait for the head: one workgroup takes its
            // update by panel k0 as the left-looking prologue of the diagonal kernel (K = 256) and factors it
            // -- launched while the machine is still empty (the bulk update of panel k0 starts at the same
            // moment on the other queue), it does not queue for a slot behind the update's first generation
            // of workgroups (55 us at N = 8192); the head then leaves that 64 x 64 tile alone.  Whole potrf,
            // without / with: N = 8192 6.54 / 6.47 ms, N = 16384 30.05 / 29.75; with carried rows it costs
            // (8.53 -> 8.82 ms with 2050 rows: the rows' queues then see an even busier chain), so not there.
            const bool head0 = !rows && w == CIMRGP_NB && gemm_uses_tile64(n - k1, wn, false);
            if (head0) {
                const int sw0 = (int)((wn < SB) ? wn : SB);
                hipLaunchKernelGGL((k_diag64q<T>), dim3(1), dim3(Q_NT), 0, sp, k + k1 * ld + k1, ld, sw0,
                                   (const T*)(k + k1 * ld + k0), (int)w, ws + (k1 / SB) * (SB * SB), info, (int)k1, (int64_t)0, (int64_t)0,
                                   (int64_t)0, no_riders<T>());
                CIMRGP_LAUNCH_CHECK("cimrgp_potrf");
            }
            GemmBatch ghead; ghead.skip_first = head0 ? 1 : 0;
            rc = gemm_nt_sub<T>(k + k1 * ld + k1, ld, k + k1 * ld + k0, ld, k + k1 * ld + k0, ld,
                                n - k1, wn, (int)w, false, sp, ghead);
            if (rc) return rc;
            // (The bulk update does not wait for the head: with the four-wave chain kernels that order no longer pays --
            // head first above 4608 rows against never: N = 8192 6.72 against 6.56 ms, HISTORY.md, round 2.)
            rc = factor_panel<T>(k, n, ld, ws, info, k1, wn, sp, false, head0);
            if (rc) return rc;
            ev_panel = la->ev[ne++];
            CIMRGP_HIP_TRY(hipEventRecord(ev_panel, sp), "hipEventRecord");
        }
        if (k1 < n) {
            // bulk: lower SYRK beyond the next panel, concurrently with the chain.  While that far
            // region is big, it is updated once per GROUP of 2-4 panels with K = 256 x group size
            // (adjacent panels are adjacent columns, the same kernel applies): fewer passes over C.
            ev_rest = nullptr;
            bool split_far = false;                // the split far update records its own events
            if (n > k2) {
                CIMRGP_HIP_TRY(hipStreamWaitEvent(sb, ev_final, 0), "hipStreamWaitEvent");
                const int64_t wnn = (n - k2 < CIMRGP_NB) ? (n - k2) : CIMRGP_NB;   // panel after next
                const int64_t k3 = k2 + wnn;
                if (grp.g0 < 0) {
                    const int64_t far_pair_above = knobs().far_pair_above;
                    const int g = group_size(n - k3, far_pair_above);
                    if (g > 1) { grp.g0 = k0; grp.left = g; }
                }
                if (grp.g0 >= 0) {
                    // a panel of a group: the columns of the panel after next with all the group's
                    // panels so far (all the chain's next head update needs -- it may start as soon
                    // as they are done) ...
                    const int kk = (int)(k1 - grp.g0);
                    rc = gemm_nt_sub<T>(k + k2 * ld + k2, ld, k + k2 * ld + grp.g0, ld, k + k2 * ld + grp.g0, ld,
                                        n - k2, wnn, kk, false, sb);
                    if (rc) return rc;
                    ev_rest = la->ev[ne++];
                    CIMRGP_HIP_TRY(hipEventRecord(ev_rest, sb), "hipEventRecord");
                    ev_bulk_last = ev_rest;
                    split_far = true;
                    if (--grp.left == 0 || n <= k3) {
                        // ... and, closing the group, the big remainder with K = 256 x group size,
                        // which overlaps the chain's next panels
                        if (n > k3) {
                            const double mm = (double)(n - k3);
                            hipEvent_t rec = rec_open(sb, mm * (mm + 1.0) * (double)kk, (mm * (mm + 1.0) + mm * (double)kk) * (double)sizeof(T));
                            rc = gemm_nt_sub<T>(k + k3 * ld + k3, ld, k + k3 * ld + grp.g0, ld, k + k3 * ld + grp.g0, ld,
                                                n - k3, n - k3, kk, true, sb, bulk_gb);
                            if (rec) (void)hipEventRecord(rec, sb);
                            if (rc) return rc;
                            ev_bulk_last = la->ev[ne++];
                            CIMRGP_HIP_TRY(hipEventRecord(ev_bulk_last, sb), "hipEventRecord");
                        }
                        grp = PanelGroup();
                    }
                } else {
                    const double mm = (double)(n - k2);
                    hipEvent_t rec = rec_open(sb, mm * (mm + 1.0) * (double)w, (mm * (mm + 1.0) + mm * (double)w) * (double)sizeof(T));
                    rc = gemm_nt_sub<T>(k + k2 * ld + k2, ld, k + k2 * ld + k0, ld, k + k2 * ld + k0, ld,
                                        n - k2, n - k2, (int)w, true, sb, bulk_gb);
                    if (rec) (void)hipEventRecord(rec, sb);
                    if (rc) return rc;
                }
                if (!split_far) {
                    ev_rest = la->ev[ne++];
                    CIMRGP_HIP_TRY(hipEventRecord(ev_rest, sb), "hipEventRecord");
                    ev_bulk_last = ev_rest;
                }
            }
        }
        rc = rows_after_panel(k0, k1, ev_final);
        if (rc) return rc;
    }
    if (rows) {
        if (ev_rows_far) CIMRGP_HIP_TRY(hipStreamWaitEvent(la->rows, ev_rows_far, 0), "hipStreamWaitEvent");
        hipEvent_t ev_rows_done = la->ev[ne++];
        CIMRGP_HIP_TRY(hipEventRecord(ev_rows_done, la->rows), "hipEventRecord");
        CIMRGP_HIP_TRY(hipStreamWaitEvent(st, ev_rows_done, 0), "hipStreamWaitEvent");
    }
    // join: the last panel (side stream); every bulk update precedes it through the chain's waits
    if (!tail_done) {
        CIMRGP_HIP_TRY(hipStreamWaitEvent(st, ev_panel, 0), "hipStreamWaitEvent");
        if (sb != st && ev_bulk_last) CIMRGP_HIP_TRY(hipStreamWaitEvent(st, ev_bulk_last, 0), "hipStreamWaitEvent");
    }
    return build_invT<T>(k, n, ld, ws, st);
    };   // body
    const int rc_body = body();
    if (rc_body == 0) {
        // (a failed record only costs the next call its early panels)
        if (la->last_done == nullptr && hipEventCreateWithFlags(&la->last_done, hipEventDisableTiming) != hipSuccess) la->last_done = nullptr;
        if (la->last_done != nullptr) (void)hipEventRecord(la->last_done, st);
    }
    if (rc_body != 0) {
        // failed enqueue: the caller's stream waits for everything that did get queued (errors of the join itself
        // cannot improve on the one being reported)
        size_t je = la->ev.size() - 4;
        for (hipStream_t q : {la->side, la->bulk, la->rows, la->rows_far}) {
            if (q == nullptr) continue;
            hipEvent_t ev = la->ev[je++];
            if (hipEventRecord(ev, q) == hipSuccess) (void)hipStreamWaitEvent(st, ev, 0);
        }
    }
    return rc_body;
}

// `bt.count` equal-sized factorisations (the blocks of one layer) in the SAME launches: every
// kernel of the one-queue sweep runs with grid.y = count, so a layer of many small blocks costs the
// host one block's worth of launches and the device sees all the blocks' panel chains side by side.
template <typename T>
int potrf_batched_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb, PotrfBatch bt,
                      hipStream_t st)
{
    if (bt.count < 1 || bt.count >= 65536) return fail("cimrgp_potrf_batched", "batch count out of range");
    hipError_t e = hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)bt.count, st);
    if (e != hipSuccess) return check_hip(e, "cimrgp_potrf_batched", "hipMemsetAsync(info)");
    // A big batch fills the machine with its panel solves already: the updates then keep launches of their own
    // (128-tiles, more efficient than 64-tile riders); riders pay where the chain's launches leave units idle.
    const bool ride = (int64_t)bt.count * (n / TR) <= knobs().fused_max_chain_wgs;
    if (!ride && bt.count >= knobs().batch_halves_min && n > CIMRGP_NB) {
        // Two halves of the batch on two queues: nothing orders them against each other, so the latency-bound
        // panel chains of one half run beside the MFMA-bound updates of the other (one queue alternates
        // between the two kinds of work and leaves the matrix cores idle for a third of a 128 x 2048 layer).
        LookAhead* la = acquire_ctx(st);
        if (la != nullptr) {
            std::lock_guard<std::mutex> guard(la->enqueue);
            if (!grow_events(la, 2)) return fail("cimrgp_potrf_batched", "hipEventCreate failed");
            PotrfBatch h0 = bt, h1 = bt;
            h0.count = bt.count / 2;
            h1.count = bt.count - h0.count;
            const int64_t c = h0.count;
            CIMRGP_HIP_TRY(hipEventRecord(la->ev[0], st), "hipEventRecord");
            CIMRGP_HIP_TRY(hipStreamWaitEvent(la->side, la->ev[0], 0), "hipStreamWaitEvent");
            int rc = panel_sweep<T, true>(k, n, ld, ws, info, b, m, ldb, st, h0);
            if (!rc) rc = build_invT<T>(k, n, ld, ws, st, h0);
            if (!rc) rc = panel_sweep<T, true>(k + c * bt.sk, n, ld, ws + c * bt.sws, info + c, b ? b + c * bt.sb : b, m, ldb, la->side, h1);
            if (!rc) rc = build_invT<T>(k + c * bt.sk, n, ld, ws + c * bt.sws, la->side, h1);
            // (joined even after a failed enqueue: the caller's stream must not run ahead of the side queue)
            CIMRGP_HIP_TRY(hipEventRecord(la->ev[1], la->side), "hipEventRecord");
            CIMRGP_HIP_TRY(hipStreamWaitEvent(st, la->ev[1], 0), "hipStreamWaitEvent");
            return rc;
        }
    }
    int rc = ride ? fused_sweep<T>(k, n, ld, ws, info, b, m, ldb, bt, st) : panel_sweep<T, true>(k, n, ld, ws, info, b, m, ldb, st, bt);
    return rc ? rc : build_invT<T>(k, n, ld, ws, st, bt);
}

template <typename T>
int solve_rows_run(const T* l, int64_t n, int64_t ld, const T* ws, T* b, int64_t m, int64_t ldb, hipStream_t st, PotrfBatch bt)
{
    if (bt.count < 1 || bt.count >= 65536) return fail("cimrgp_trsm_rows", "batch count out of range");
    return panel_sweep<T, false>(const_cast<T*>(l), n, ld, const_cast<T*>(ws), nullptr, b, m, ldb, st, bt);
}

template int potrf_run<double>(double*, int64_t, int64_t, double*, int32_t*, double*, int64_t, int64_t, hipStream_t, hipStream_t);
template int potrf_run<float>(float*, int64_t, int64_t, float*, int32_t*, float*, int64_t, int64_t, hipStream_t, hipStream_t);
template int potrf_batched_run<double>(double*, int64_t, int64_t, double*, int32_t*, double*, int64_t, int64_t, PotrfBatch, hipStream_t);
template int potrf_batched_run<float>(float*, int64_t, int64_t, float*, int32_t*, float*, int64_t, int64_t, PotrfBatch, hipStream_t);
template int solve_rows_run<double>(const double*, int64_t, int64_t, const double*, double*, int64_t, int64_t, hipStream_t, PotrfBatch);
template int solve_rows_run<float>(const float*, int64_t, int64_t, const float*, float*, int64_t, int64_t, hipStream_t, PotrfBatch);

}  // namespace cimrgp
