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
// rows, inverses, the gate); this file is the host schedule that launches them:
//
//   Problem<T>              what is being factored (matrix, workspace, info, carried rows, batch)
//   panel_chain             the five launches of one panel (diag_launch: the first of them)
//   trailing_update         one lower trailing update, with its profiling record
//   rows_solve_panel, rows_panel_step     the carried rows: one panel's solve; solve + (grouped) updates on one queue
//   panel_sweep             one queue, updates in launches of their own (big batches, cimrgp_trsm_rows)
//   plan_riders, fused_sweep              one queue, updates riding in the chain's launches (n <= 5120, tails, small batches)
//   LookAheadRun<T>         n > 5120: the look-ahead schedule on a context's queues, one method per phase --
//                           start, early_panels, gated_step / ungated_step per panel, tail (hand-off to fused_sweep),
//                           rows_after_panel (rows_grouped / rows_pipelined), join
//   potrf_run               chooses the context, locks it, runs the steps, joins the queues if one failed
#include "common.hpp"
#include "chain_kernels.hpp"
#include "rows_kernels.hpp"
#include <cstdlib>
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
static hipEvent_t rec_open(hipStream_t st, double flops, double bytes)
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

#define CIMRGP_HIP_TRY(fn, call, what) \
    do { hipError_t e__ = (call); if (e__ != hipSuccess) return check_hip(e__, fn, what); } while (0)

constexpr int64_t ROWS_PAIR_ABOVE_SOLVE = 1024;   // stand-alone row-wise solve: pair the updates while more columns remain
// (the factorisation's thresholds are `knobs()`, common.hpp: constants in the product build)

// The factorisation (or row-wise solve) being enqueued.
template <typename T>
struct Problem {
    T* k;                 // the matrix (row-major, lower triangle), n x n, leading dimension ld
    int64_t n, ld;
    T* ws;                // workspace: 64x64 inverses, then the 256x256 invT blocks and the pair blocks (build_invT)
    int32_t* info;
    T* b;                 // carried rows (m x n, leading dimension ldb) solved along, or nullptr
    int64_t m, ldb;
    PotrfBatch bt;        // equal-sized problems in the same launches (grid.y; strides of k, ws, b)

    bool rows() const { return b != nullptr && m > 0; }
    T* inv64(int64_t c0) const { return ws + (c0 / SB) * (SB * SB); }   // inverse of the diagonal block at column c0
};

// Width of the panel that starts at column k0 (0 at or past the end: only the last panel is ragged).
static inline int64_t panel_width(int64_t n, int64_t k0)
{
    return (n - k0 < CIMRGP_NB) ? (n - k0) : CIMRGP_NB;
}

// How many panels share one pass over the far part of the matrix being updated (K = 256 x that
// many), once that far part is larger than `pair_above`.  Stand-alone rate of the update at
// K = 256 / 512 / 768 / 1024: 51.5 / 59.0 / 62.1 / 63.5 TF/s at M = 15360, 55.5 / 62.1 / 64.3 / 65.3
// TF/s at M = 32256.  Inside the factorisation (whole potrf, groups capped at 1 / 2 / 3 / 4):
// N = 32768: 217.8 / 203.9 / 201.3 / 200.9 ms, N = 65536: 1650 / 1512 / 1505 / 1505 ms (56.9 -> 62.3
// TF/s) -- pairs bring most of it.  At N = 8192 pairing (thresholds 2048..6144) raises the update
// kernel's rate (49 -> 56 % of peak) but not the end-to-end time (longer-lived update workgroups,
// longer slot waits of the chain), so the factorisation's threshold (Knobs::far_pair_above) lies above
// that size.  The group is also kept small enough for the operand panel (far x K x 8 bytes) to fit
// the 256 MB Infinity Cache, which caps it at 3 (a group of 4 would need far > 32768 and far <= 32768
// at once).
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

// The first 64-column diagonal block of a panel, at column c0 and sw wide, in a launch of its own: the
// left-looking prologue takes the kp columns at `lr` (the block's rows), riders `rd` come along as extra
// workgroups.  `waves4`: the four-wave kernel (panel_chain).
template <typename T>
static int diag_launch(const Problem<T>& p, int64_t c0, int sw, const T* lr, int kp, const Riders<T>& rd, bool waves4,
                       hipStream_t st)
{
    const dim3 grid((unsigned)(1 + rd.total), (unsigned)p.bt.count);
    if (waves4)
        hipLaunchKernelGGL((k_diag64q<T>), grid, dim3(Q_NT), 0, st,
                           p.k + c0 * p.ld + c0, p.ld, sw, lr, kp, p.inv64(c0), p.info, (int)c0, p.bt.sk, p.bt.sws, p.bt.sb, rd);
    else
        hipLaunchKernelGGL((k_diag64<T>), grid, dim3(DG_NT), 0, st,
                           p.k + c0 * p.ld + c0, p.ld, sw, lr, kp, p.inv64(c0), p.info, (int)c0, p.bt.sk, p.bt.sws, p.bt.sb, rd);
    CIMRGP_LAUNCH_CHECK("cimrgp_potrf");
    return 0;
}

// The latency-bound chain of one panel [k0, k0 + w) on stream st: the first 64-column diagonal
// block in a launch of its own, then one k_link per further sub-block (panel solve of sub-block s
// beside the factorisation of diagonal block s + 1), and the panel solve of the last sub-block.
// The carried rows of `p`, if any, are solved along (second row set).
// `alone`: nothing heavy runs beside the chain (one-queue sweeps, the tail).  Then the nine-wave
// kernels are used (a few per cent faster by themselves: N = 2048 1.05 against 1.09 ms).  Beside a
// running trailing update a nine-wave workgroup is dispatched only to a compute unit BOTH of whose
// update workgroups have retired -- in effect after the update's last generation (first link of a
// panel 230-300 us at N = 8192) -- while a four-wave workgroup fits beside one update workgroup and
// gets, by queue priority, the first slot that falls free: there the four-wave forms run
// (N = 8192: period of the update-bound panels 437 / 391 / 371 -> 405 / 363 / 355 us).
// `first_done`: the caller has launched the first diagonal block itself (LookAheadRun: ahead of the head update).
// `riders`: nullptr, or the update tiles riding in the chain's launches -- riders[0] in the first diagonal
// block's launch, riders[1..3] in the links, riders[4] in the last sub-block's panel solve (fused_sweep).
// `left64`: the first diagonal block takes, as its left-looking prologue, the 64 columns just left of the
// panel (the previous panel's last sub-block, whose contribution the riders could not apply before it was final).
template <typename T>
static int panel_chain(const Problem<T>& p, int64_t k0, int64_t w, hipStream_t st, bool alone,
                       bool first_done = false, const Riders<T>* riders = nullptr, bool left64 = false)
{
    const char* fn = "cimrgp_potrf";
    T* const kmat = p.k;
    const int64_t n = p.n, ld = p.ld;
    const PotrfBatch& bt = p.bt;
    // (a batch of factorisations in one launch is its own crowd: many link workgroups compete for the
    // compute units, and the four-wave form packs twice as many of them)
    const bool waves4 = !alone || bt.count > 1;
    const bool rows = p.rows();
    T* const b = rows ? p.b : (T*)nullptr;
    const int m = rows ? (int)p.m : 0;
    const unsigned nbatch = (unsigned)bt.count;
    const int64_t k1 = k0 + w;
    // rows per panel-solve workgroup: groups of TRSM_GROUP tiles in batched launches (k_linkq / k_trsm64 take it as an argument)
    const int trg = (bt.count > 1 && waves4) ? TR * TRSM_GROUP : TR;
    const int nb2 = rows ? (int)((p.m + trg - 1) / trg) : 0;
    const Riders<T> none = no_riders<T>();
    int launch = 0;                                   // 0: first diagonal block, 1..3: links, 4: last panel solve
    for (int64_t c0 = k0; c0 < k1; c0 += SB) {
        const int sw = (int)((k1 - c0 < SB) ? (k1 - c0) : SB);
        const int kprev = (int)(c0 - k0);
        const int64_t pc = c0 + sw;            // first row after this sub-block
        const T* lrow = kmat + c0 * ld + k0;   // rows of the diagonal block, earlier panel columns
        if (c0 == k0 && !first_done) {
            int rc = diag_launch<T>(p, c0, sw, left64 ? lrow - SB : lrow, left64 ? (int)SB : kprev, riders ? riders[0] : none, waves4, st);
            if (rc) return rc;
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
                                   kmat, ld, (int)n, (int)c0, (int)k0, wn, rows ? b + c0 : (T*)nullptr, p.ldb, m,
                                   p.ws, p.info, bt.sk, bt.sws, bt.sb, nchain, rd, trg);
            else
                hipLaunchKernelGGL((k_link<T>), dim3((unsigned)(nchain + rd.total), nbatch), dim3(DG_NT), 0, st,
                                   kmat, ld, (int)n, (int)c0, (int)k0, wn, rows ? b + c0 : (T*)nullptr, p.ldb, m,
                                   p.ws, p.info, bt.sk, bt.sws, bt.sb, nchain, rd);
            CIMRGP_LAUNCH_CHECK(fn);
            continue;
        }
        // the last sub-block (pc == k1): its panel solve
        const int64_t m1 = n - pc;
        const int nb1 = (int)((m1 + trg - 1) / trg);
        const Riders<T>& rd = riders ? riders[4] : none;
        if (nb1 + nb2 + rd.total > 0) {
            hipLaunchKernelGGL((k_trsm64<T>), dim3((unsigned)(nb1 + nb2 + rd.total), nbatch), dim3(256), 0, st,
                               kmat + pc * ld + c0, ld, (int)m1, nb1,
                               rows ? b + c0 : (T*)nullptr, p.ldb, m,
                               sw, kprev, lrow, ld, (const T*)p.inv64(c0), bt.sk, bt.sws, bt.sb, nb1 + nb2, rd, trg);
            CIMRGP_LAUNCH_CHECK(fn);
        }
    }
    return 0;
}

// The lower trailing update  C -= A A^T  with C = the lower triangle from row and column c0 on (M = n - c0) and
// A = the K = kk columns from a0 on of the same rows, on `st`; `gb`: how gemm_nt runs it (persistent units, head
// tiles first, the batch).  While profiling is on the launch is bracketed by a record: M (M + 1) K flop and its
// algorithmic traffic -- C (lower) read and written, the panel once -- per problem of the batch.
template <typename T>
static int trailing_update(const Problem<T>& p, int64_t c0, int64_t a0, int kk, hipStream_t st, GemmBatch gb = GemmBatch())
{
    const double mm = (double)(p.n - c0);
    hipEvent_t rec = rec_open(st, mm * (mm + 1.0) * (double)kk * (double)gb.count,
                              (mm * (mm + 1.0) + mm * (double)kk) * (double)sizeof(T) * (double)gb.count);
    T* const rows_c0 = p.k + c0 * p.ld;
    int rc = gemm_nt_sub<T>(rows_c0 + c0, p.ld, rows_c0 + a0, p.ld, rows_c0 + a0, p.ld, p.n - c0, p.n - c0, kk, true, st, gb);
    if (rec) (void)hipEventRecord(rec, st);
    return rc;
}

// The rows' solve of one full panel [r0, r0 + 256): k_rows_step, with the previous panel's update of these columns
// fused in (`with_prev`: the caller left it out of its updates) or as the solve alone.
template <typename T>
static int rows_step_launch(const Problem<T>& p, int64_t r0, bool with_prev, hipStream_t st, const char* fn)
{
    const PotrfBatch& bt = p.bt;
    // (a batch: blockIdx.y = matrix, strides of the rows' arena, the matrices and the workspaces)
    const dim3 grid((unsigned)((p.m + RowsStep<T>::R - 1) / RowsStep<T>::R), (unsigned)bt.count);
    if (with_prev)
        hipLaunchKernelGGL((k_rows_step<T, true>), grid, dim3(256), 0, st, p.b + r0, p.ldb, (int)p.m,
                           (const T*)(p.k + r0 * p.ld + (r0 - CIMRGP_NB)), p.ld, (const T*)p.inv64(r0),
                           (const T*)nullptr, (int64_t)0, 0, 1, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0, bt.sb, bt.sk, bt.sws);
    else
        hipLaunchKernelGGL((k_rows_step<T, false>), grid, dim3(256), 0, st, p.b + r0, p.ldb, (int)p.m,
                           (const T*)(p.k + r0 * p.ld + r0), p.ld, (const T*)p.inv64(r0),
                           (const T*)nullptr, (int64_t)0, 0, 1, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0, bt.sb, bt.sk, bt.sws);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

// The carried rows' solve of panel r0 on `st`.  A full panel: one k_rows_step (until round 4 a 64-tile update and
// k_trsm256, two latency-bound launches).  A ragged last panel: k_trsm256, behind the previous panel's update of its
// columns when that is still owed (`near_pending`; cannot happen: the promise is made for full panels only).
template <typename T>
static int rows_solve_panel(const Problem<T>& p, int64_t r0, bool near_pending, hipStream_t st, const char* fn)
{
    const int64_t rw = panel_width(p.n, r0);
    if (p.m > 0 && rw == CIMRGP_NB) return rows_step_launch<T>(p, r0, near_pending, st, fn);
    const PotrfBatch& bt = p.bt;
    if (near_pending) {
        GemmBatch gb; gb.count = bt.count; gb.sc = gb.sa = bt.sb; gb.sb = bt.sk;
        int rcn = gemm_nt_sub<T>(p.b + r0, p.ldb, p.b + r0 - CIMRGP_NB, p.ldb, p.k + r0 * p.ld + r0 - CIMRGP_NB, p.ld,
                                 p.m, rw, CIMRGP_NB, false, st, gb);
        if (rcn) return rcn;
    }
    hipLaunchKernelGGL((k_trsm256<T>), dim3((unsigned)((p.m + TR - 1) / TR), (unsigned)bt.count), dim3(256), 0, st,
                       p.b + r0, p.ldb, (int)p.m, (int)rw, (const T*)(p.k + r0 * p.ld + r0), p.ld,
                       (const T*)p.inv64(r0), bt.sb, bt.sk, bt.sws);
    CIMRGP_LAUNCH_CHECK(fn);
    return 0;
}

// One panel of a row-wise solve  B <- B L^-T  on one queue: the 256-wide solve of the panel's columns, then
// the update of the columns right of it.  While more than `pair_above` columns lie beyond the
// next panel, the far columns are updated once per GROUP of panels with K = 256 x group size
// (fewer passes over B): every panel of a group but the last only updates the next panel's
// columns (with all the group's panels so far), the last one everything right of itself
// (adjacent panels are adjacent columns of B and of L).
template <typename T>
static int rows_panel_step(const Problem<T>& p, int64_t r0, PanelGroup& grp, int64_t pair_above, hipStream_t st, const char* fn)
{
    T* const b = p.b;
    const T* const lmat = p.k;
    const int64_t n = p.n, ld = p.ld, m = p.m, ldb = p.ldb;
    const int64_t rw = panel_width(n, r0);
    const int64_t r1 = r0 + rw;
    GemmBatch gb; gb.count = p.bt.count; gb.sc = gb.sa = p.bt.sb; gb.sb = p.bt.sk;
    const bool near_pending = grp.near_pending;
    grp.near_pending = false;
    int rcs = rows_solve_panel<T>(p, r0, near_pending, st, fn);
    if (rcs) return rcs;
    if (n <= r1) { grp = PanelGroup(); return 0; }
    const int64_t rn = panel_width(n, r1);
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

// One pass over the panels on one queue, every update in a launch of its own.  With FACTOR the matrix
// itself is factored and the carried rows, if any, go through the same panel operations, which turns
// them into  B L^-T; without it the matrix is a finished factor and only the rows are solved.
template <typename T, bool FACTOR>
static int panel_sweep(const Problem<T>& p, hipStream_t st)
{
    const char* fn = FACTOR ? "cimrgp_potrf" : "cimrgp_trsm_rows";
    const int64_t n = p.n;
    const bool rows = p.rows();
    PanelGroup rows_grp;
    for (int64_t k0 = 0; k0 < n; k0 += CIMRGP_NB) {
        const int64_t w = panel_width(n, k0);
        const int64_t k1 = k0 + w;
        if (!FACTOR && rows) {
            int rc = rows_panel_step<T>(p, k0, rows_grp, ROWS_PAIR_ABOVE_SOLVE, st, fn);
            if (rc) return rc;
            continue;
        }
        if (FACTOR) {
            int rcc = panel_chain<T>(p, k0, w, st, true);
            if (rcc) return rcc;
        }
        if (n > k1) {
            if (FACTOR) {
                GemmBatch gb; gb.count = p.bt.count; gb.sc = gb.sa = gb.sb = p.bt.sk;
                int rc = trailing_update<T>(p, k1, k0, (int)w, st, gb);
                if (rc) return rc;
            }
            if (rows) {
                GemmBatch gb; gb.count = p.bt.count; gb.sc = gb.sa = p.bt.sb; gb.sb = p.bt.sk;
                int rc = gemm_nt_sub<T>(p.b + k1, p.ldb, p.b + k0, p.ldb, p.k + k1 * p.ld + k0, p.ld,
                                        p.m, n - k1, (int)w, false, st, gb);
                if (rc) return rc;
            }
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// One-queue factorisation with the updates riding in the chain's launches (round 3; "Riders" in chain_kernels.hpp).
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
    std::vector<hipEvent_t>* ev = nullptr;   // the context's event pool and the caller's position in it
    size_t* ne = nullptr;
    int cus = 0;
    int64_t min_rows = 1 << 30;          // FAR on the bulk queue while n - k2 >= min_rows
    // called once per panel [k0, k1) after its chain has been enqueued, with an event that says "panel final"
    // (carried rows that follow the factorisation on queues of their own: LookAheadRun::rows_after_panel)
    int (*on_final)(void* ctx, int64_t k0, int64_t k1, hipEvent_t ev_final) = nullptr;
    void* ctx = nullptr;

    hipEvent_t next_event() const { return (*ev)[(*ne)++]; }
};

static inline int64_t tiles64(int64_t v) { return (v + 63) / 64; }

template <typename T>
static void add_rider(Riders<T>& r, const RiderJob<T>& jb)
{
    if (jb.count <= 0) return;
    r.job[r.njobs++] = jb;
    r.total += jb.count;
}

// Rider job  C (mm x nn) -= A (mm x kk) B (nn x kk)^T, all of its 64 x 64 tiles.
template <typename T>
static RiderJob<T> rect_job(T* c, int64_t ldc, const T* a, int64_t lda, const T* bb, int64_t ldbb, int64_t mm, int64_t nn, int64_t kk)
{
    RiderJob<T> jb;
    jb.c = c; jb.a = a; jb.b = bb; jb.ldc = ldc; jb.lda = lda; jb.ldb = ldbb;
    jb.m = (int)mm; jb.n = (int)nn; jb.k = (int)kk; jb.lower = 0; jb.tiles_n = (int)tiles64(nn);
    jb.first = 0; jb.count = (int)(tiles64(mm) * tiles64(nn)); jb.skip00 = 0; jb.rows_job = 0;
    return jb;
}

// Where the K = 256 rider tiles of the previous panel's update go in the five launches of a panel's chain.
struct RiderPlan {
    int64_t near0 = 0;                                   // NEAR(prev) tiles [0, near0) ride in launch 0, the rest in launch 1
    int64_t far_first[5] = {0, 0, 0, 0, 0}, far_count[5] = {0, 0, 0, 0, 0};     // FAR(prev) tiles of each launch
    int64_t rows_first[5] = {0, 0, 0, 0, 0}, rows_count[5] = {0, 0, 0, 0, 0};   // the carried rows' far tiles of each launch
};

// K = 256 rider tiles a launch has room for: `rounds` rounds of the slots its own chain workgroups leave, less
// the riders placed already (`fixed`, in K = 256 tile equivalents).
static inline int64_t rider_capacity(int rounds, int slots, int nchain, int fixed)
{
    const int64_t c = (int64_t)rounds * (slots - nchain) - fixed;
    return c > 0 ? c : 0;
}

// Plans the riders of panel [k0, k0 + w) (next panel wn > 0 wide, m_rows carried rows solved along by the chain):
// how many of the near_tiles + far_tiles + rows_far_tiles K = 256 tiles each launch takes.  `busy_cus`: compute
// units held by a persistent FAR on a second queue; ph3_tiles (K = 64) and rows_near_tiles ride in launch 0 already.
// A launch's riders run in ROUNDS of (2 workgroups per compute unit - the launch's own chain workgroups),
// ~20 us per round of K = 256 tiles, and a launch lasts max(its chain part, its rounds): whole rounds are given
// to the launches whose chain part they lengthen least (a launch with 1.3 rounds of riders
// takes two rounds' time: the first version of this schedule, split by the chain parts'
// durations, took 221 us per panel at 4352 trailing rows where 7 packed rounds take ~150).
// Round 4: a launch starts with NO round of K = 256 riders; rounds go first to the launches whose
// chain part outlasts a round anyway (the links), and the first diagonal kernel and the last solve --
// 15 and 13 us alone, 25-29 and 16 with a round of riders -- take riders only when the links are full
// (HISTORY.md, round 4).
static RiderPlan plan_riders(int64_t n, int64_t k0, int64_t w, int64_t wn, int64_t m_rows, int busy_cus,
                             int64_t ph3_tiles, int64_t rows_near_tiles, int64_t near_tiles, int64_t far_tiles, int64_t rows_far_tiles)
{
    // the chain parts of the five launches last about this long alone (us; round 4, as measured in the tail of an
    // N = 8192 factorisation without riders' help)
    static const double chain_us[5] = {15.0, 21.0, 24.0, 28.0, 13.0};
    const int slots = 2 * (256 - busy_cus);
    const double t_round = (double)knobs().rider_round_us;
    const int64_t k1 = k0 + w;
    int nchain[5], fixed[5];
    for (int i = 0; i < 5; ++i) {
        // rows the launch's panel solve covers: below diagonal block i + 1 (links), below the panel (last solve)
        const int64_t below = (i == 4) ? n - k1 : n - k0 - SB * (i + 1);
        nchain[i] = (i == 0) ? 1 : (int)((below + TR - 1) / TR) + (i < 4 ? 1 : 0) + (int)((m_rows + TR - 1) / TR);
        fixed[i] = 0;
    }
    // riders already placed (PH3, ROWS in launch 0; this panel's PH(p, s) go to launches 2..4: K = 64 tiles,
    // about a third of a K = 256 tile each)
    fixed[0] = (int)(ph3_tiles / 3 + rows_near_tiles);
    if (w == CIMRGP_NB) for (int i = 2; i < 5; ++i) fixed[i] = (int)near_tiles / 3;
    int rounds[5] = {0, 0, 0, 0, 0};
    int64_t cap[5];
    const int64_t need = near_tiles + far_tiles + rows_far_tiles;
    for (;;) {
        int64_t cap_all = 0;
        for (int i = 0; i < 5; ++i) { cap[i] = rider_capacity(rounds[i], slots, nchain[i], fixed[i]); cap_all += cap[i]; }
        // NEAR must fit launches 0 and 1
        const bool near_ok = cap[0] + cap[1] >= near_tiles;
        if (cap_all >= need && near_ok) break;
        int best = -1;
        double best_cost = 1e30;
        for (int i = 0; i < (near_ok ? 5 : 2); ++i) {
            const double now = (rounds[i] * t_round > chain_us[i]) ? rounds[i] * t_round : chain_us[i];
            const double then = ((rounds[i] + 1) * t_round > chain_us[i]) ? (rounds[i] + 1) * t_round : chain_us[i];
            const double cost = (then - now) / (double)(slots - nchain[i]);
            if (cost < best_cost - 1e-12) { best_cost = cost; best = i; }
        }
        ++rounds[best];
        if (rounds[best] > 64) {                   // cannot happen (guards the loop)
            for (int i = 0; i < 5; ++i) cap[i] = rider_capacity(rounds[i], slots, nchain[i], fixed[i]);
            break;
        }
    }
    RiderPlan plan;
    // NEAR(prev): launches 0 and 1 only (from launch 2 on this panel's sub-blocks update the same columns); the
    // first link before the diagonal kernel (the capacities cover it: near_ok)
    if (near_tiles > cap[1]) plan.near0 = near_tiles - cap[1];
    // FAR(prev), then the carried rows' far update, over the launches' remaining capacities; the last launch in
    // this order takes whatever is left
    int64_t done_f = 0, done_r = 0;
    static const int order[5] = {1, 2, 3, 0, 4};
    for (int oi = 0; oi < 5; ++oi) {
        const int i = order[oi];
        int64_t room = cap[i] - (i == 0 ? plan.near0 : i == 1 ? (near_tiles - plan.near0) : 0);
        if (room < 0) room = 0;
        int64_t take_f = far_tiles - done_f;
        if (oi < 4 && take_f > room) take_f = room;
        room -= take_f;
        int64_t take_r = rows_far_tiles - done_r;
        if (oi < 4 && take_r > room) take_r = (room > 0 ? room : 0);
        plan.far_first[i] = done_f;  plan.far_count[i] = take_f;
        plan.rows_first[i] = done_r; plan.rows_count[i] = take_r;
        done_f += take_f;
        done_r += take_r;
    }
    return plan;
}

template <typename T>
static int fused_sweep(const Problem<T>& p, hipStream_t st, int64_t k_begin = 0, int64_t prev_w = 0, const FarBulk* fb = nullptr)
{
    const char* fn = "cimrgp_potrf";
    T* const kmat = p.k;
    T* const b = p.b;
    const int64_t n = p.n, ld = p.ld, m = p.m, ldb = p.ldb;
    const bool rows = p.rows();
    hipEvent_t ev_prev_final = nullptr;                     // (far-bulk mode) panel `prev` is final, on st
    hipEvent_t ev_far_last = nullptr;                       // (far-bulk mode) the last FAR launched on the bulk queue
    if (fb && prev_w > 0) {
        ev_prev_final = fb->next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_prev_final, st), "hipEventRecord");
    }
    int64_t q0 = (prev_w > 0) ? k_begin - prev_w : -1;      // previous panel (-1: none)
    int64_t qw = prev_w;
    bool ph3_pending = false;                                // prev's last sub-block still owed to this panel's columns
    bool rows_pending = false;                               // ROWS(prev) owed (at a tail entry the rows have seen prev already)
    for (int64_t k0 = k_begin; k0 < n; k0 += CIMRGP_NB) {
        const int64_t w = panel_width(n, k0);
        const int64_t k1 = k0 + w;
        const int64_t wn = panel_width(n, k1);
        const int64_t k2 = k1 + wn;
        Riders<T> rd[5];
        for (int i = 0; i < 5; ++i) rd[i] = no_riders<T>();
        bool far_launched = false;
        if (q0 >= 0) {
            const T* pa = kmat + q0;                          // prev's panel columns, row r at pa + r * ld
            if (ph3_pending) {
                // prev's last 64 columns -> this panel's columns, every row from k0 (tile (0,0) is workgroup 0's)
                RiderJob<T> jb = rect_job<T>(kmat + k0 * ld + k0, ld, kmat + k0 * ld + (k0 - SB), ld, kmat + k0 * ld + (k0 - SB), ld,
                                             n - k0, w, SB);
                jb.skip00 = 1;
                add_rider(rd[0], jb);
            }
            const int64_t ph3_tiles = rd[0].total;            // K = 64 tiles
            int64_t rows_near_tiles = 0, rows_far_tiles = 0;
            if (rows_pending) {
                // the carried rows' columns of THIS panel: needed by the panel's first link (which solves them)
                RiderJob<T> jb = rect_job<T>(b + k0, ldb, b + q0, ldb, pa + k0 * ld, ld, m, w, qw);
                jb.rows_job = 1;
                add_rider(rd[0], jb);
                rows_near_tiles = jb.count;
                if (wn > 0) rows_far_tiles = tiles64(m) * tiles64(n - k1);      // ... and everything right of it: any launch
            }
            if (wn > 0) {
                const int64_t near_tiles = tiles64(n - k1) * tiles64(wn);
                const int64_t tf = (n > k2) ? tiles64(n - k2) : 0;
                // FAR(prev) on the bulk queue (persistent, fb->cus units) while it is large; as riders otherwise
                const bool far_on_bulk = fb && fb->cus >= 8 && ev_prev_final && p.bt.count == 1 && n - k2 >= fb->min_rows && (n - k2) % 128 == 0 &&
                                         qw == CIMRGP_NB && gemm_pers_head_tiles(n - k2, (int)qw, (int)sizeof(T)) > 0;
                if (far_on_bulk) {
                    CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(fb->bulk, ev_prev_final, 0), "hipStreamWaitEvent");
                    GemmBatch gb; gb.pers = fb->cus; gb.pers_force = 1;
                    int rcf = trailing_update<T>(p, k2, q0, (int)qw, fb->bulk, gb);
                    if (rcf) return rcf;
                    far_launched = true;
                }
                const int64_t far_tiles = far_on_bulk ? 0 : tf * (tf + 1) / 2;
                const RiderPlan plan = plan_riders(n, k0, w, wn, rows ? m : 0, far_on_bulk ? fb->cus : 0,
                                                   ph3_tiles, rows_near_tiles, near_tiles, far_tiles, rows_far_tiles);
                RiderJob<T> nr = rect_job<T>(kmat + k1 * ld + k1, ld, pa + k1 * ld, ld, pa + k1 * ld, ld, n - k1, wn, qw);
                RiderJob<T> n0 = nr; n0.first = 0; n0.count = (int)plan.near0; add_rider(rd[0], n0);
                RiderJob<T> n1 = nr; n1.first = (int)plan.near0; n1.count = (int)(near_tiles - plan.near0); add_rider(rd[1], n1);
                RiderJob<T> fr;
                fr.c = kmat + k2 * ld + k2; fr.a = pa + k2 * ld; fr.b = pa + k2 * ld; fr.ldc = fr.lda = fr.ldb = ld;
                fr.m = fr.n = (int)(n - k2); fr.k = (int)qw; fr.lower = 1; fr.tiles_n = (int)tf; fr.skip00 = 0; fr.rows_job = 0;
                fr.first = 0; fr.count = 0;
                RiderJob<T> rf = fr;
                if (rows_far_tiles > 0) {
                    rf = rect_job<T>(b + k1, ldb, b + q0, ldb, pa + k1 * ld, ld, m, n - k1, qw);
                    rf.rows_job = 1;
                }
                for (int i = 0; i < 5; ++i) {
                    if (plan.far_count[i] > 0) { RiderJob<T> part = fr; part.first = (int)plan.far_first[i]; part.count = (int)plan.far_count[i]; add_rider(rd[i], part); }
                    if (plan.rows_count[i] > 0) { RiderJob<T> part = rf; part.first = (int)plan.rows_first[i]; part.count = (int)plan.rows_count[i]; add_rider(rd[i], part); }
                }
            }
        }
        if (wn > 0 && w == CIMRGP_NB) {
            // this panel's sub-blocks 0, 1, 2 -> the next panel's columns, each as soon as it is final
            for (int sblk = 0; sblk < 3; ++sblk) {
                const int64_t cs = k0 + SB * sblk;
                add_rider(rd[2 + sblk], rect_job<T>(kmat + k1 * ld + k1, ld, kmat + k1 * ld + cs, ld, kmat + k1 * ld + cs, ld, n - k1, wn, SB));
            }
        }
        if (fb) {
            // the FAR launched during the previous iteration wrote the columns this chain's riders (and, when FAR
            // rides again, its FAR tiles) are about to touch
            if (ev_far_last) {
                CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_far_last, 0), "hipStreamWaitEvent");
                ev_far_last = nullptr;
            }
            if (far_launched) {
                ev_far_last = fb->next_event();
                CIMRGP_HIP_TRY(fn, hipEventRecord(ev_far_last, fb->bulk), "hipEventRecord");
            }
        }
        int rc = panel_chain<T>(p, k0, w, st, true, false, rd, ph3_pending);
        if (rc) return rc;
        if (fb && (k1 < n || fb->on_final)) {
            ev_prev_final = fb->next_event();
            CIMRGP_HIP_TRY(fn, hipEventRecord(ev_prev_final, st), "hipEventRecord");
            if (fb->on_final) {
                rc = fb->on_final(fb->ctx, k0, k1, ev_prev_final);
                if (rc) return rc;
            }
        }
        q0 = k0;
        qw = w;
        ph3_pending = (wn > 0 && w == CIMRGP_NB);
        rows_pending = rows && k1 < n;
        // a ragged panel that still has columns to its right cannot happen (only the last panel is ragged)
    }
    if (fb && ev_far_last) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_far_last, 0), "hipStreamWaitEvent");
    return 0;
}

// ---------------------------------------------------------------------------
// Look-ahead contexts.  A factorisation with look-ahead (LookAheadRun below) uses queues beside the caller's
// stream, forks and joins them by events only, and takes the events from a pool.  Queues, pool and the gate's
// device counter form a context; there is one per caller stream that factors (at most MAX_CTX per device,
// created on first use), so that independent factorisations enqueued on different streams run side by side.
// ---------------------------------------------------------------------------
namespace {
constexpr int MAX_CTX = 8;               // look-ahead contexts per device: one per concurrently factoring caller stream
constexpr int64_t SINGLE_QUEUE_MAX = 5120;   // n at or below this: one queue, no look-ahead (see potrf_run)

struct LookAhead {
    hipStream_t side = nullptr;        // panel chain (high priority, all compute units)
    hipStream_t rows = nullptr;        // carried rows: lags behind the factorisation
    hipStream_t rows_far = nullptr;    // carried rows: far part of each panel's update (beside the rows' own panel chain)
    std::vector<hipEvent_t> ev;
    int* flag = nullptr;               // device counter: head tiles stored by the combined update launches (k_gate polls it)
    hipStream_t owner = nullptr;       // the caller stream this context was created for
    bool gate_ok = false;              // this context may hold a kernel that waits for another one (k_gate): the device's first context only
    std::mutex enqueue;                // one factorisation at a time enqueues on this context's queues
    hipEvent_t last_done = nullptr;    // behind the latest look-ahead factorisation on this context (recorded on its caller's stream)
};
constexpr size_t CTX_QUEUES = 3;       // side, rows, rows_far (the trailing updates run on the caller's stream)
std::mutex g_reg_mutex;                // guards g_ctx and context creation
std::vector<LookAhead*> g_ctx[16];     // per device; contexts live as long as the process

// Streams of one context.  Chain and rows queue or none: a context without its rows queue would have to
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
    // (the carried rows' second queue is created on first use: LookAheadRun::start)
    if (!ok) {
        if (la->side) (void)hipStreamDestroy(la->side);
        if (la->rows) (void)hipStreamDestroy(la->rows);
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
            for (hipStream_t q : {la->side, la->rows, la->rows_far})
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
// last third of a factorisation runs on one queue, LookAheadRun::tail): the front end of the NEXT independent block can run
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

// Workspace layout: [ceil(n/64) slabs of 64x64 inverses][ceil(n/256) blocks of 256x256 invT][pair blocks].
template <typename T>
static int build_invT(const Problem<T>& p, hipStream_t st)
{
    const char* fn = "cimrgp_potrf";
    const T* const kmat = p.k;
    T* const ws = p.ws;
    const int64_t n = p.n, ld = p.ld;
    const PotrfBatch& bt = p.bt;
    const int64_t npan = (n + CIMRGP_NB - 1) / CIMRGP_NB;
    T* invT = ws + ws_invT_offset(n);
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

// ---------------------------------------------------------------------------
// Factorisation with one-panel look-ahead (n > SINGLE_QUEUE_MAX), enqueued once on the queues of context `la`.
// The trailing update of panel p is split into the columns of panel p+1 ("head", rectangular) and the rest (lower
// SYRK).  As soon as the head is done, panel p+1 is factored on a second, high-priority queue while the caller's
// stream is still busy with the rest; the latency-bound panel chain (64 sequential columns per diagonal block)
// hides behind the MFMA-bound update for as long as the trailing matrix is large.
// The chain queue runs the whole latency-bound chain in queue order -- "head" update of the
// next panel's columns, then that panel's factorisation -- so that no inter-queue signal
// sits between two links of the chain; the caller's stream runs the bulk of each trailing
// update.  Cross-queue edges: "panel final" (chain -> caller's stream, before the bulk update that reads it)
// and "bulk update done" (caller's stream -> chain, before the next head touches columns the bulk update wrote).
// The carried rows follow on queues of their own (rows_after_panel).  Fork and join by events only.
//
// The members are the state the steps share; enqueue() is the schedule:
//   start, early_panels, then per panel  tail (once, ends the loop) | gated_step | ungated_step,  then join.
// ---------------------------------------------------------------------------
namespace {
template <typename T>
struct LookAheadRun {
    static constexpr const char* fn = "cimrgp_potrf";
    const Problem<T> p;                  // the factorisation with its carried rows
    const Problem<T> pk;                 // ... and the matrix alone: what the chain queue and the tail's sweep factor
    const int64_t n;
    LookAhead* const la;
    const hipStream_t st;                // the caller's stream: bulk updates, the tail, the join
    const hipStream_t sp;                // the chain queue (la->side)
    const bool early;                    // the first panel follows the caller's writes on the chain queue (potrf_run: ready_on)
    // The device counter of the gate belongs to the CONTEXT, and beyond MAX_CTX contexts a context serves caller
    // streams other than its owner (acquire_ctx, by hash).  Only the owner's factorisations may reset and count on
    // it: a second caller stream would reset the counter under the owner's in-flight gates (which then expire) and
    // have its own gates satisfied by the owner's tiles (a silently wrong factor).  Everybody else keeps the head
    // update on the chain queue (round 2's schedule), which needs no counter.
    const bool may_gate;
    const bool rows;                     // carried rows to solve along
    bool rows_pipeline = false;          // the rows' far updates have a queue of their own (set by start)
    // Bulk updates beside the chain: the persistent update kernel on all compute units but `chain_cus`,
    // which stay free for the chain's kernels (one persistent workgroup fills a unit's registers, so the
    // grid size IS the split).
    GemmBatch bulk_gb;
    size_t ne = 0;                       // events of la->ev handed out so far
    int flag_expected = 0;               // head tiles the chain has been told to wait for so far
    hipEvent_t ev_start = nullptr;       // the caller's stream at the start of this factorisation
    hipEvent_t ev_panel = nullptr;       // the latest panel factored on the chain queue is final
    hipEvent_t ev_rest = nullptr;        // bulk update of the previous panel (what the next head must wait for), or nullptr
    PanelGroup grp;                      // open group of panels whose far update is still owed
    bool tail_done = false;              // the tail ran: the caller's stream holds the end of the factorisation already
    int64_t k_begin = 0;                 // first panel of the look-ahead loop (behind the early panels)
    // trailing columns below which the carried rows start (early_panels sets it again: beside the previous
    // factorisation's last panels the rows do better starting two panels later)
    int64_t rows_start;
    int64_t rows_next = 0;               // first panel the carried rows have not seen yet
    PanelGroup rows_grp;                 // carried rows: open group of panels whose far update is owed
    hipEvent_t ev_rows_far = nullptr;    // carried rows: last far update queued on the second rows queue
    hipEvent_t ev_rows_far_prev = nullptr;   // ... and the one before it

    LookAheadRun(const Problem<T>& prob, LookAhead* ctx, hipStream_t stream, bool early_start)
        : p(prob), pk{prob.k, prob.n, prob.ld, prob.ws, prob.info, nullptr, 0, 0, PotrfBatch()}, n(prob.n), la(ctx), st(stream),
          sp(ctx->side), early(early_start), may_gate(ctx->gate_ok && ctx->owner == stream), rows(prob.rows()),
          rows_start(knobs().rows_start_below)
    {
        if (knobs().gemm_pers > 0 && knobs().chain_cus > 0 && knobs().chain_cus < knobs().gemm_pers)
            bulk_gb.pers = knobs().gemm_pers - knobs().chain_cus;
    }

    hipEvent_t next_event() { return la->ev[ne++]; }
    // one panel's chain on the chain queue (panel_chain: `alone`, `first_done`)
    int chain(int64_t k0, int64_t w, bool alone, bool first_done = false) { return panel_chain<T>(pk, k0, w, sp, alone, first_done); }

    // Fork: the chain queue behind the caller's stream (unless `early`), the first panel, "panel 0 final".
    int start()
    {
        if (may_gate) CIMRGP_HIP_TRY(fn, hipMemsetAsync(la->flag, 0, 256, st), "hipMemsetAsync(flag)");
        ev_start = next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_start, st), "hipEventRecord");
        if (!early) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sp, ev_start, 0), "hipStreamWaitEvent");
        int rc = chain(0, panel_width(n, 0), true);
        if (rc) return rc;
        ev_panel = next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_panel, sp), "hipEventRecord");
        // second rows queue: created when first wanted (cimrgp_set_rows_queues(1) before the first
        // factorisation with carried rows means it never exists: a process then holds four streams)
        if (rows && rows_queues() == 2 && la->rows_far == nullptr) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&la->rows_far, hipStreamNonBlocking, lo) != hipSuccess) la->rows_far = nullptr;
        }
        rows_pipeline = (rows_queues() == 2) && la->rows_far != nullptr;
        return 0;
    }

    // `early` only: knobs().early_panels more panels one-queue style (update of everything right of panel p, then panel
    // p+1, in queue order on the chain queue): work of THIS factorisation done while the previous one's tail leaves the
    // machine two-thirds idle.  From panel k_begin on the look-ahead steps take over, behind `st` as always.
    // (only while the context's previous factorisation is still in flight when this one is enqueued: with the machine
    //  to itself a factorisation is better off with look-ahead from the first panel on)
    int early_panels()
    {
        if (!early) return 0;
        const bool prev_in_flight = la->last_done != nullptr && hipEventQuery(la->last_done) == hipErrorNotReady;
        (void)hipGetLastError();                     // "not ready" is an answer, not an error for the launch checks below to find
        const int np_early = (sizeof(T) == 8 && prev_in_flight) ? knobs().early_panels : 0;
        GemmBatch early_gb = bulk_gb;
        if (knobs().early_cus >= 8) early_gb.pers = knobs().early_cus;
        for (int i = 0; i < np_early; ++i) {
            const int64_t k0 = (int64_t)i * CIMRGP_NB, k1 = k0 + CIMRGP_NB;
            if (n - k1 < 4 * CIMRGP_NB || (n - k1) % 128 != 0) break;
            int rc = trailing_update<T>(pk, k1, k0, (int)CIMRGP_NB, sp, early_gb);
            if (rc) return rc;
            rc = chain(k1, CIMRGP_NB, true);
            if (rc) return rc;
            k_begin = k1;
        }
        if (k_begin > 0) {
            rows_start = knobs().rows_start_below_early;
            ev_panel = next_event();
            CIMRGP_HIP_TRY(fn, hipEventRecord(ev_panel, sp), "hipEventRecord");
        }
        CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sp, ev_start, 0), "hipStreamWaitEvent");
        return 0;
    }

    // With carried rows (round 3): the last rows_beside_tail_below columns are factored by the same one-queue fused
    // sweep while the rows keep following on their own queues, one panel behind (the sweep tells them when a
    // panel is final).  Entered later than the tail without rows (2560 against 4864 trailing columns): while the
    // rows' far updates are large the sweep's riders would queue behind them for compute units (113 posteriors/s
    // entered at 4864 and 107 at 6144 against 117.3 without and 119.4 at 2560).
    bool rows_beside_tail() const { return rows && knobs().rows_beside_tail_below > 0; }

    // Panel k0 (factored, not the last) is where the single-queue tail starts.
    bool tail_starts(int64_t k0) const
    {
        const int64_t k1 = k0 + panel_width(n, k0);
        if (k1 >= n || grp.g0 >= 0) return false;
        return rows_beside_tail() ? n - k1 <= knobs().rows_beside_tail_below : (!rows && n - k1 <= knobs().tail_below);
    }

    // ---- single-queue tail.  Once the trailing matrix is small the look-ahead no longer
    // pays: its chain kernels wait for slots beside the update and every panel costs an
    // inter-queue hop, while one queue runs 4 x (diag + solve) = 124 us plus ONE update of
    // everything right of the panel, all at full speed (measured whole potrf, single queue
    // vs look-ahead: n = 2048: 1.23 vs 1.37 ms, 4096: 2.80 vs 3.04, 6144: 4.84 vs 5.05,
    // 8192: 7.95 vs 7.73; hybrid at N = 8192: 7.86 -> 7.52 ms).  With carried rows the rows'
    // own queue fills the tail either way and the hybrid is neutral (9.69 vs 9.73 ms): not
    // used then (but see rows_beside_tail).  Panel k0 is factored; the region right of it holds all earlier
    // panels' updates once the caller's stream, which ran them, has passed "panel k0 final".
    // Round 3: the tail is the fused one-queue sweep -- the head update of panel k0 (the next panel's
    // columns, all rows) in a launch of its own, everything after it rides in the chains' launches
    // (fused_sweep).  (Carried rows that caught up here and then rode along: HISTORY.md, round 3.)
    int tail(int64_t k0)
    {
        const int64_t w = panel_width(n, k0), k1 = k0 + w;
        const bool rows_beside = rows_beside_tail();
        CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_panel, 0), "hipStreamWaitEvent");
        if (rows_beside) {
            // the carried rows keep following on their own queues (panel k0 here, the tail's panels from the sweep)
            int rc = rows_after_panel(k0, k1, ev_panel);
            if (rc) return rc;
        }
        T* const rows_k1 = p.k + k1 * p.ld;
        int rc = gemm_nt_sub<T>(rows_k1 + k1, p.ld, rows_k1 + k0, p.ld, rows_k1 + k0, p.ld,
                                n - k1, panel_width(n, k1), (int)w, false, st);
        if (rc) return rc;
        FarBulk fbk;
        fbk.bulk = sp;                              // the chain's queue of the look-ahead phase is free now
        fbk.ev = &la->ev;
        fbk.ne = &ne;
        fbk.cus = knobs().tail_far_cus;
        fbk.min_rows = knobs().tail_far_min_rows;
        if (rows_beside) {
            fbk.cus = 0;                            // far updates as riders: the rows' far updates hold the persistent units
            fbk.on_final = &LookAheadRun::rows_after_tail_panel;
            fbk.ctx = this;
        }
        const bool use_fb = rows_beside || (!rows && fbk.cus >= 8 && knobs().gemm_pers >= 8);
        rc = fused_sweep<T>(pk, st, k1, w, use_fb ? &fbk : nullptr);
        if (rc) return rc;
        tail_done = true;
        return 0;
    }
    static int rows_after_tail_panel(void* self, int64_t k0, int64_t k1, hipEvent_t ev_final)
    {
        return static_cast<LookAheadRun*>(self)->rows_after_panel(k0, k1, ev_final);
    }

    // Head tiles of a gated step for panel k0, or 0: the ungated step.
    // (not while the carried rows are running: their kernels hold compute units the persistent workgroups
    // of the combined launch -- head tiles included -- would have to wait for: 114 -> 109 posteriors/s)
    // (measured again in round 5 with the rows on 192 units: 137.2 -> 135.4 / 134.3 posteriors/s, HISTORY.md)
    int gate_heads(int64_t k0) const
    {
        const int64_t w = panel_width(n, k0), k1 = k0 + w;
        const int64_t wn = panel_width(n, k1), k2 = k1 + wn;
        const bool rows_running = rows && (n - k1 <= rows_start);
        if (!may_gate || rows_running || w != CIMRGP_NB || wn != CIMRGP_NB || n <= k2 || grp.g0 >= 0) return 0;
        if (group_size(n - k2 - panel_width(n, k2), knobs().far_pair_above) != 1) return 0;
        return gemm_pers_head_tiles(n - k1, (int)w, (int)sizeof(T));
    }

    // Round 3: head and bulk update of panel k0 as ONE persistent launch on the caller's stream.  Its first
    // tiles are the next panel's columns (the old "head": on the chain's queue it ran on the few compute
    // units the persistent bulk update leaves free -- 144 us for 1 Gflop at N = 8192, the longest link of
    // the chain); they are counted as they are stored and the chain waits for the count through a
    // one-workgroup gate kernel.  The next panel's first diagonal block does not wait: it takes its own
    // 64 x 64 update as its prologue (as before) and the rest of the first 128 x 128 tile along as riders.
    int gated_step(int64_t k0, int heads)
    {
        const int64_t w = panel_width(n, k0), k1 = k0 + w;
        const int64_t wn = panel_width(n, k1);
        const hipEvent_t ev_final = ev_panel;          // panel k0 is final (recorded on the chain queue)
        // The persistent launch is ENQUEUED before the gate that waits for its head tiles: a tool that runs one
        // kernel at a time in submission order (rocprofv3 --pmc, HIP_LAUNCH_BLOCKING) then finds the count complete
        // when the gate runs, instead of running the gate first and timing it out.
        hipEvent_t ev_rest_prev = ev_rest;
        flag_expected += heads;
        // caller's stream: everything right of panel k0, the next panel's columns first, behind "panel k0 final" as an event.
        // (A device word posted by the chain and polled by a gate here: potrf n = 8192 5.43 -> 5.38 ms, the step
        // unchanged, and the gate sat out its watchdog under rocprofv3 --pmc -- round 5, HISTORY.md.)
        CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_final, 0), "hipStreamWaitEvent");
        GemmBatch gb = bulk_gb;
        gb.head_first = 1;
        gb.flag = la->flag;
        int rc = trailing_update<T>(pk, k1, k0, (int)w, st, gb);
        if (rc) return rc;
        ev_rest = next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_rest, st), "hipEventRecord");
        // chain queue: first diagonal block (+ the rest of tile (0, 0) of 128 as riders), gate, the other links
        if (ev_rest_prev) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sp, ev_rest_prev, 0), "hipStreamWaitEvent");
        const T* head = p.k + k1 * p.ld + k0;          // panel k0's columns, rows from k1 on
        Riders<T> r0 = no_riders<T>();
        {
            RiderJob<T>& jb = r0.job[0];
            jb.c = p.k + k1 * p.ld + k1; jb.a = head; jb.b = head; jb.ldc = jb.lda = jb.ldb = p.ld;
            jb.m = 128; jb.n = 128; jb.k = (int)w; jb.lower = 0; jb.tiles_n = 2; jb.first = 0; jb.count = 4; jb.skip00 = 1; jb.rows_job = 0;
            r0.njobs = 1; r0.total = 4;
        }
        rc = diag_launch<T>(pk, k1, (int)SB, head, (int)w, r0, true, sp);
        if (rc) return rc;
        hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, sp, (const int*)la->flag, flag_expected, p.info);
        CIMRGP_LAUNCH_CHECK(fn);
        rc = chain(k1, wn, false, true);
        if (rc) return rc;
        ev_panel = next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_panel, sp), "hipEventRecord");
        return rows_after_panel(k0, k1, ev_final);
    }

    // Panel k0 without the gate: the head update and the next panel on the chain queue, the rest of the update
    // (or a group's share of it) on the caller's stream.
    int ungated_step(int64_t k0)
    {
        const int64_t w = panel_width(n, k0), k1 = k0 + w;
        const int64_t wn = panel_width(n, k1), k2 = k1 + wn;
        const hipEvent_t ev_final = ev_panel;          // panel k0 is final (recorded on the chain queue)
        T* const k = p.k;
        const int64_t ld = p.ld;
        if (k1 < n) {
            // chain: head (columns of the next panel, all rows below), then the next panel
            if (ev_rest) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sp, ev_rest, 0), "hipStreamWaitEvent");
            // The next panel's FIRST diagonal block does not wait for the head: one workgroup takes its
            // update by panel k0 as the left-looking prologue of the diagonal kernel (K = 256) and factors it
            // -- launched while the machine is still empty (the bulk update of panel k0 starts at the same
            // moment on the other queue), it does not queue for a slot behind the update's first generation
            // of workgroups (55 us at N = 8192); the head then leaves that 64 x 64 tile alone.  Whole potrf,
            // without / with: N = 8192 6.54 / 6.47 ms, N = 16384 30.05 / 29.75; with carried rows it costs
            // (8.53 -> 8.82 ms with 2050 rows: the rows' queues then see an even busier chain), so not there.
            const bool head0 = !rows && w == CIMRGP_NB && gemm_uses_tile64(n - k1, wn, false);
            if (head0) {
                int rc = diag_launch<T>(pk, k1, (int)((wn < SB) ? wn : SB), k + k1 * ld + k0, (int)w, no_riders<T>(), true, sp);
                if (rc) return rc;
            }
            GemmBatch ghead; ghead.skip_first = head0 ? 1 : 0;
            int rc = gemm_nt_sub<T>(k + k1 * ld + k1, ld, k + k1 * ld + k0, ld, k + k1 * ld + k0, ld,
                                    n - k1, wn, (int)w, false, sp, ghead);
            if (rc) return rc;
            // (The bulk update does not wait for the head: with the four-wave chain kernels that order no longer pays --
            // head first above 4608 rows against never: N = 8192 6.72 against 6.56 ms, HISTORY.md, round 2.)
            rc = chain(k1, wn, false, head0);
            if (rc) return rc;
            ev_panel = next_event();
            CIMRGP_HIP_TRY(fn, hipEventRecord(ev_panel, sp), "hipEventRecord");
            // bulk: lower SYRK beyond the next panel, concurrently with the chain.  While that far
            // region is big, it is updated once per GROUP of 2-3 panels with K = 256 x group size
            // (adjacent panels are adjacent columns, the same kernel applies): fewer passes over C.
            ev_rest = nullptr;
            if (n > k2) {
                CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_final, 0), "hipStreamWaitEvent");
                const int64_t wnn = panel_width(n, k2);   // panel after next
                const int64_t k3 = k2 + wnn;
                if (grp.g0 < 0) {
                    const int g = group_size(n - k3, knobs().far_pair_above);
                    if (g > 1) { grp.g0 = k0; grp.left = g; }
                }
                if (grp.g0 >= 0) {
                    // a panel of a group: the columns of the panel after next with all the group's
                    // panels so far (all the chain's next head update needs -- it may start as soon
                    // as they are done) ...
                    const int kk = (int)(k1 - grp.g0);
                    rc = gemm_nt_sub<T>(k + k2 * ld + k2, ld, k + k2 * ld + grp.g0, ld, k + k2 * ld + grp.g0, ld,
                                        n - k2, wnn, kk, false, st);
                    if (rc) return rc;
                    ev_rest = next_event();
                    CIMRGP_HIP_TRY(fn, hipEventRecord(ev_rest, st), "hipEventRecord");
                    if (--grp.left == 0 || n <= k3) {
                        // ... and, closing the group, the big remainder with K = 256 x group size,
                        // which overlaps the chain's next panels
                        if (n > k3) {
                            rc = trailing_update<T>(pk, k3, grp.g0, kk, st, bulk_gb);
                            if (rc) return rc;
                        }
                        grp = PanelGroup();
                    }
                } else {
                    rc = trailing_update<T>(pk, k2, k0, (int)w, st, bulk_gb);
                    if (rc) return rc;
                    ev_rest = next_event();
                    CIMRGP_HIP_TRY(fn, hipEventRecord(ev_rest, st), "hipEventRecord");
                }
            }
        }
        return rows_after_panel(k0, k1, ev_final);
    }

    // Panel [k0, k1) is final (event ev_final): solve + update the carried rows.  They form their own
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
    int rows_after_panel(int64_t k0, int64_t k1, hipEvent_t ev_final)
    {
        if (!rows) return 0;
        if (n - k1 > rows_start && k1 < n) return 0;
        CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(la->rows, ev_final, 0), "hipStreamWaitEvent");
        // (pairing the rows' updates below rows_pair_above was measured neutral-to-worse at N = 8192)
        for (int64_t r0 = rows_next; r0 <= k0; r0 += CIMRGP_NB) {
            const int64_t r1 = r0 + panel_width(n, r0);
            const int64_t r2 = r1 + panel_width(n, r1);        // first column beyond the next panel
            const bool grouped = !rows_pipeline || rows_grp.g0 >= 0 || (n > r2 && group_size(n - r2, knobs().rows_pair_above) > 1);
            int rc = grouped ? rows_grouped(r0) : rows_pipelined(r0);
            if (rc) return rc;
        }
        rows_next = k1;
        return 0;
    }

    // grouped far updates (large matrices): the rows' chain as one queue
    int rows_grouped(int64_t r0)
    {
        hipStream_t sq = la->rows;
        if (ev_rows_far) { CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sq, ev_rows_far, 0), "hipStreamWaitEvent"); ev_rows_far = nullptr; }
        return rows_panel_step<T>(p, r0, rows_grp, knobs().rows_pair_above, sq, "cimrgp_potrf_rows");
    }

    // The rows' own chain on `sq`: panel r0's solve with the previous panel's update of its columns fused in
    // (rows_solve_panel); the update of everything beyond the next panel (the bulk of the flops) on a second
    // queue.  far(p) needs the solved columns of panel p only and writes the columns from panel p+2 on: the step
    // of panel p+2 waits for it, the step of panel p+1 does not.
    int rows_pipelined(int64_t r0)
    {
        hipStream_t sq = la->rows;                     // always present (make_ctx: both queues or no context)
        T* const b = p.b;
        T* const k = p.k;
        const int64_t ld = p.ld, ldb = p.ldb, m = p.m;
        const int64_t rw = panel_width(n, r0);
        const int64_t r1 = r0 + rw;
        const int64_t rn = panel_width(n, r1);
        const bool near_pending = rows_grp.near_pending;
        rows_grp.near_pending = false;
        if (near_pending && ev_rows_far_prev) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sq, ev_rows_far_prev, 0), "hipStreamWaitEvent");
        int rcr = rows_solve_panel<T>(p, r0, near_pending, sq, "cimrgp_potrf_rows");
        if (rcr) return rcr;
        if (n <= r1) return 0;
        hipEvent_t ev_w = next_event();
        CIMRGP_HIP_TRY(fn, hipEventRecord(ev_w, sq), "hipEventRecord");
        if (rw == CIMRGP_NB && rn == CIMRGP_NB) {
            rows_grp.near_pending = true;
        } else {
            if (ev_rows_far) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sq, ev_rows_far, 0), "hipStreamWaitEvent");
            rcr = gemm_nt_sub<T>(b + r1, ldb, b + r0, ldb, k + r1 * ld + r0, ld, m, rn, (int)rw, false, sq);
            if (rcr) return rcr;
        }
        ev_rows_far_prev = ev_rows_far;
        if (n > r1 + rn) {
            hipStream_t sf = la->rows_far;
            CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(sf, ev_w, 0), "hipStreamWaitEvent");
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
            ev_rows_far = next_event();
            CIMRGP_HIP_TRY(fn, hipEventRecord(ev_rows_far, sf), "hipEventRecord");
        }
        return 0;
    }

    // Join: the rows' queues, then the last panel (chain queue; every bulk update precedes it through the
    // chain's waits), into the caller's stream; the inverses follow there.
    int join()
    {
        if (rows) {
            if (ev_rows_far) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(la->rows, ev_rows_far, 0), "hipStreamWaitEvent");
            hipEvent_t ev_rows_done = next_event();
            CIMRGP_HIP_TRY(fn, hipEventRecord(ev_rows_done, la->rows), "hipEventRecord");
            CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_rows_done, 0), "hipStreamWaitEvent");
        }
        if (!tail_done) CIMRGP_HIP_TRY(fn, hipStreamWaitEvent(st, ev_panel, 0), "hipStreamWaitEvent");
        return build_invT<T>(pk, st);
    }

    int enqueue()
    {
        int rc = start();
        if (!rc) rc = early_panels();
        if (rc) return rc;
        for (int64_t k0 = k_begin; k0 < n; k0 += CIMRGP_NB) {
            if (tail_starts(k0)) {
                rc = tail(k0);                 // ... which factors everything from panel k0 on
                if (rc) return rc;
                break;
            }
            const int heads = gate_heads(k0);
            rc = (heads > 0) ? gated_step(k0, heads) : ungated_step(k0);
            if (rc) return rc;
        }
        return join();
    }
};
}  // namespace

template <typename T>
int potrf_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb, hipStream_t st, hipStream_t ready_on)
{
    const char* fn = "cimrgp_potrf";
    const Problem<T> p{k, n, ld, ws, info, b, m, ldb, PotrfBatch()};
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
    CIMRGP_HIP_TRY(fn, hipMemsetAsync(info, 0, sizeof(int32_t), early ? la->side : st), "hipMemsetAsync(info)");
    if (la == nullptr) {
        int rc0 = fused_sweep<T>(p, st);
        return rc0 ? rc0 : build_invT<T>(p, st);
    }

    // Host threads whose streams share a context serialise their ENQUEUE (microseconds); distinct
    // caller streams have distinct contexts and enqueue concurrently.
    std::lock_guard<std::mutex> guard(la->enqueue);
    // Events of one factorisation: at most four per panel (two of its look-ahead step or of its tail panel, two of
    // the carried rows' step) and five more (start, first panel, early panels, tail entry, rows done); the last
    // CTX_QUEUES of the pool are kept for the join after a failure.  The request leaves more than twice that.
    if (!grow_events(la, (size_t)(9 * npanels + 16) + CTX_QUEUES)) return fail(fn, "hipEventCreate failed");
    LookAheadRun<T> run(p, la, st, early);
    const int rc = run.enqueue();
    if (rc == 0) {
        // (a failed record only costs the next call its early panels)
        if (la->last_done == nullptr && hipEventCreateWithFlags(&la->last_done, hipEventDisableTiming) != hipSuccess) la->last_done = nullptr;
        if (la->last_done != nullptr) (void)hipEventRecord(la->last_done, st);
        return 0;
    }
    // Failed enqueue.  The steps enqueue on several queues, and an error return in the middle must not leave the
    // caller's stream running ahead of work already queued on them (the caller may free or reuse K / workspace / B):
    // the caller's stream waits for everything that did get queued (errors of the join itself cannot improve on the
    // one being reported).
    size_t je = la->ev.size() - CTX_QUEUES;
    for (hipStream_t q : {la->side, la->rows, la->rows_far}) {
        if (q == nullptr) continue;
        hipEvent_t ev = la->ev[je++];
        if (hipEventRecord(ev, q) == hipSuccess) (void)hipStreamWaitEvent(st, ev, 0);
    }
    return rc;
}

// `bt.count` equal-sized factorisations (the blocks of one layer) in the SAME launches: every
// kernel of the one-queue sweep runs with grid.y = count, so a layer of many small blocks costs the
// host one block's worth of launches and the device sees all the blocks' panel chains side by side.
template <typename T>
int potrf_batched_run(T* k, int64_t n, int64_t ld, T* ws, int32_t* info, T* b, int64_t m, int64_t ldb, PotrfBatch bt,
                      hipStream_t st)
{
    if (bt.count < 1 || bt.count >= 65536) return fail("cimrgp_potrf_batched", "batch count out of range");
    CIMRGP_HIP_TRY("cimrgp_potrf_batched", hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)bt.count, st), "hipMemsetAsync(info)");
    const Problem<T> p{k, n, ld, ws, info, b, m, ldb, bt};
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
            Problem<T> h0 = p, h1 = p;
            h0.bt.count = bt.count / 2;
            h1.bt.count = bt.count - h0.bt.count;
            const int64_t c = h0.bt.count;
            h1.k += c * bt.sk; h1.ws += c * bt.sws; h1.info += c;
            if (h1.b) h1.b += c * bt.sb;
            CIMRGP_HIP_TRY("cimrgp_potrf", hipEventRecord(la->ev[0], st), "hipEventRecord");
            CIMRGP_HIP_TRY("cimrgp_potrf", hipStreamWaitEvent(la->side, la->ev[0], 0), "hipStreamWaitEvent");
            int rc = panel_sweep<T, true>(h0, st);
            if (!rc) rc = build_invT<T>(h0, st);
            if (!rc) rc = panel_sweep<T, true>(h1, la->side);
            if (!rc) rc = build_invT<T>(h1, la->side);
            // (joined even after a failed enqueue: the caller's stream must not run ahead of the side queue)
            CIMRGP_HIP_TRY("cimrgp_potrf", hipEventRecord(la->ev[1], la->side), "hipEventRecord");
            CIMRGP_HIP_TRY("cimrgp_potrf", hipStreamWaitEvent(st, la->ev[1], 0), "hipStreamWaitEvent");
            return rc;
        }
    }
    int rc = ride ? fused_sweep<T>(p, st) : panel_sweep<T, true>(p, st);
    return rc ? rc : build_invT<T>(p, st);
}

template <typename T>
int solve_rows_run(const T* l, int64_t n, int64_t ld, const T* ws, T* b, int64_t m, int64_t ldb, hipStream_t st, PotrfBatch bt)
{
    if (bt.count < 1 || bt.count >= 65536) return fail("cimrgp_trsm_rows", "batch count out of range");
    const Problem<T> p{const_cast<T*>(l), n, ld, const_cast<T*>(ws), nullptr, b, m, ldb, bt};
    return panel_sweep<T, false>(p, st);
}

template int potrf_run<double>(double*, int64_t, int64_t, double*, int32_t*, double*, int64_t, int64_t, hipStream_t, hipStream_t);
template int potrf_run<float>(float*, int64_t, int64_t, float*, int32_t*, float*, int64_t, int64_t, hipStream_t, hipStream_t);
template int potrf_batched_run<double>(double*, int64_t, int64_t, double*, int32_t*, double*, int64_t, int64_t, PotrfBatch, hipStream_t);
template int potrf_batched_run<float>(float*, int64_t, int64_t, float*, int32_t*, float*, int64_t, int64_t, PotrfBatch, hipStream_t);
template int solve_rows_run<double>(const double*, int64_t, int64_t, const double*, double*, int64_t, int64_t, hipStream_t, PotrfBatch);
template int solve_rows_run<float>(const float*, int64_t, int64_t, const float*, float*, int64_t, int64_t, hipStream_t, PotrfBatch);

}  // namespace cimrgp
