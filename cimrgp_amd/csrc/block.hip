// The staged-call bookkeeping behind cimrgp_block_posterior[_staged]: the records of calls in flight, their safety nets and
// the three-stage call itself.  The entry points and their checks are in api.hip; declarations in common.hpp.
#include "common.hpp"
#include <mutex>

namespace cimrgp {
// (layer.hip) the targets as carried rows, rows[c][j] = y[j][c]; and back: z[j][c] = alpha[j][c] = rows[c][j]
template <typename T> int rhs_rows_run(const T* y, int64_t n, int q, T* rows, int64_t ldr, hipStream_t st);
template <typename T> int rows_to_z_run(const T* rows, int64_t ldr, int64_t n, int q, T* z, T* alpha, hipStream_t st, T* work = nullptr);

// cimrgp_block_posterior: the separate entry points' work in one call, in their order.  (Measured and not kept: the
// Gram matrix right of the first panel and the carried rows written BESIDE the first panel's chain -- the chain's
// first diagonal block then took 59-64 us instead of 16-20 under the write traffic and the step got no shorter:
// HISTORY.md.)
// Staged calls in flight, per device (round 5: one record per (stream, stream_solve) PAIR -- round 4 kept one record
// per device, so two caller stream pairs on one device overwrote each other's and lost both safety nets below).
// A record = the latest staged call of its pair: an event (created once per slot) recorded behind its solve stage and
// the call's whole buffer set (k, w, workspace, alpha, z, scratch: the solve stage reads or writes every one of them).
struct StagedRec_ {
    hipStream_t st = nullptr, solve = nullptr;
    hipEvent_t event = nullptr;
    hipEvent_t prev_event = nullptr;           // behind the solve stage of the pair's call BEFORE the latest (has_prev)
    bool has_prev = false;
    bool live = false;
    unsigned long long age = 0;
    const void* buf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
constexpr int STAGED_DEVS = 16, STAGED_RECS = 32, STAGED_RING = 64;
struct StagedDev_ {
    std::mutex m;
    StagedRec_ rec[STAGED_RECS];
    unsigned long long clock = 0;
    hipEvent_t ring[STAGED_RING] = {};          // hand-over events between a call's stages
    unsigned ring_next = 0;
};
static StagedDev_* staged_devs_() { static StagedDev_ a[STAGED_DEVS]; return a; }

// cimrgp_shutdown: the events above (idle devices only: the caller has synchronised)
int staged_shutdown_()
{
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (int d = 0; d < STAGED_DEVS; ++d) {
        StagedDev_& sd = staged_devs_()[d];
        std::lock_guard<std::mutex> guard(sd.m);
        bool any = false;
        for (auto& r : sd.rec) any = any || r.event != nullptr || r.prev_event != nullptr;
        for (auto& e : sd.ring) any = any || e != nullptr;
        if (!any) continue;
        (void)hipSetDevice(d);
        for (auto& r : sd.rec) { if (r.event) (void)hipEventDestroy(r.event); if (r.prev_event) (void)hipEventDestroy(r.prev_event); r = StagedRec_(); }
        for (auto& e : sd.ring) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
    if (have_cur) (void)hipSetDevice(cur);
    return 0;
}

template <typename T>
int block_posterior_typed(const void* x, int64_t n, int d, const void* y, int q, const void* xs, int64_t ns, double ell, double sf2,
                          double noise, void* k, int64_t ldk, void* ws, int32_t* info, void* w, int64_t ldw, void* alpha, void* z,
                          void* scratch, void* mean, void* var, int add_noise, int accumulate,
                          hipStream_t s_front, hipStream_t st, hipStream_t s_solve)
{
    using namespace cimrgp;
    const char* fn = "cimrgp_block_posterior";
    T* wt = (T*)w;
    int dev_id = 0;                                   // the events below belong to the device they were created on
    if (hipGetDevice(&dev_id) != hipSuccess || dev_id < 0 || dev_id >= STAGED_DEVS) dev_id = 0;
    StagedDev_& sd = staged_devs_()[dev_id];
    // `to` continues where `from` stands now (an event that lives until both have passed it)
    auto hand_over = [&](hipStream_t from, hipStream_t to) -> int {
        if (from == to) return 0;
        // a ring of events per device, created once (a wait captures the record that precedes it: an event may be
        // recorded again while an earlier wait on it is still queued)
        hipEvent_t e = nullptr;
        {
            std::lock_guard<std::mutex> guard(sd.m);
            hipEvent_t& slot = sd.ring[sd.ring_next++ % STAGED_RING];
            if (slot == nullptr) {
                hipError_t e0 = hipEventCreateWithFlags(&slot, hipEventDisableTiming);
                if (e0 != hipSuccess) { slot = nullptr; return check_hip(e0, fn, "hipEventCreate"); }
            }
            e = slot;
        }
        hipError_t e1 = hipEventRecord(e, from);
        hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(to, e, 0) : e1;
        return check_hip(e2, fn, "hipEventRecord / hipStreamWaitEvent");
    };
    const void* mine[6] = {k, w, ws, alpha, z, scratch};
    // Safety net 1: ANY buffer of a staged call whose solve stage may still be running (any pair of streams of this
    // device, a plain call on the same set included) handed in again -- one buffer set where two are needed: the
    // front end waits for that solve stage; correct results, no overlap.
    int rc = 0;
    {
        std::lock_guard<std::mutex> guard(sd.m);
        for (auto& r : sd.rec) {
            if (!r.live || r.solve == s_front || rc) continue;       // same queue: already ordered
            bool shares = false;
            for (const void* a : mine) for (const void* b : r.buf) shares = shares || (a != nullptr && a == b);
            if (shares) rc = check_hip(hipStreamWaitEvent(s_front, r.event, 0), fn, "hipStreamWaitEvent");
        }
    }
    // Safety net 3 (round 5): a front stream of its own (cimrgp_front_queue: the front end beside the PREVIOUS call's
    // factorisation) is not ordered behind anything the earlier calls did on `st`.  The latest call of the pair is covered
    // by net 1 when it shares a buffer; every call before it by one wait for the solve stage of the call before the
    // latest (the solve queue is in order, so that covers all older ones; it finished a factorisation ago: no cost).
    // Without a solve queue of its own there are no records: the front stream then simply follows `st`.
    if (!rc && s_front != st) {
        if (s_solve == st) {
            rc = hand_over(st, s_front);
        } else {
            std::lock_guard<std::mutex> guard(sd.m);
            for (auto& r : sd.rec)
                if (r.live && r.has_prev && r.st == st && r.solve == s_solve && !rc)
                    rc = check_hip(hipStreamWaitEvent(s_front, r.prev_event, 0), fn, "hipStreamWaitEvent");
        }
    }
    // front end: the Gram matrix, the cross-Gram matrix and the targets as carried rows
    if (!rc) rc = rbf_gram_run<T>((const T*)x, n, (const T*)x, n, d, ell, sf2, noise, (T*)k, ldk, true, true, s_front);
    if (!rc && ns > 0) rc = rbf_gram_run<T>((const T*)xs, ns, (const T*)x, n, d, ell, sf2, 0.0, wt, ldw, false, false, s_front);
    if (!rc) rc = rhs_rows_run<T>((const T*)y, n, q, wt + ns * ldw, ldw, s_front);
    if (!rc) rc = hand_over(s_front, st);
    if (!rc) rc = potrf_run<T>((T*)k, n, ldk, (T*)ws, info, wt, ns + q, ldw, st, s_front);
    if (!rc) rc = hand_over(st, s_solve);
    // Safety net 2: two buffer sets in rotation need no ordering by the caller: behind its factorisation `st` waits for
    // the solve stage of the PREVIOUS call on the same pair of streams (finished long ago: it ran beside this
    // factorisation), so whatever the caller enqueues on `st` next -- the front end of the call after this one, on the
    // set that solve stage read -- comes after it.
    if (!rc && s_solve != st) {
        std::lock_guard<std::mutex> guard(sd.m);
        for (auto& r : sd.rec)
            if (r.live && r.st == st && r.solve == s_solve && !rc)
                rc = check_hip(hipStreamWaitEvent(st, r.event, 0), fn, "hipStreamWaitEvent");
    }
    // z = L^-1 y (the last q carried rows), alpha = L^-T z, mean = W z, var = sf2 - sum W^2 (+ noise)
    if (!rc) rc = rows_to_z_run<T>(wt + ns * ldw, ldw, n, q, (T*)z, (T*)alpha, s_solve, (T*)scratch);
    if (!rc) rc = potrs_run<T>((const T*)k, n, ldk, (const T*)ws, (T*)alpha, q, nullptr, (T*)scratch, true, s_solve, PotrfBatch(), true);
    if (!rc && ns > 0) rc = predict_from_w_run<T>((const T*)w, ns, n, ldw, (const T*)z, q, sf2, add_noise ? noise : 0.0, nullptr, nullptr,
                                                   (T*)mean, (T*)var, accumulate, s_solve, 1, nullptr, 0);
    if (!rc && s_solve != st) {
        // this call becomes its pair's record (its slot, or a free one, or the slot of the pair idle longest -- whose
        // solve stage is waited for on the host first, so that no net is lost: 32 pairs per device, rare)
        std::lock_guard<std::mutex> guard(sd.m);
        StagedRec_* slot = nullptr;
        for (auto& r : sd.rec) if (r.live && r.st == st && r.solve == s_solve) slot = &r;
        if (slot) {
            // the pair's own record: the latest call becomes "the one before", its event is kept; the older event is recorded again
            std::swap(slot->event, slot->prev_event);
            slot->has_prev = true;
        } else {
            for (auto& r : sd.rec) if (!r.live && !slot) slot = &r;
            if (!slot) {
                slot = &sd.rec[0];
                for (auto& r : sd.rec) if (r.age < slot->age) slot = &r;
                (void)hipEventSynchronize(slot->event);
            }
            slot->has_prev = false;
        }
        if (slot->event == nullptr && hipEventCreateWithFlags(&slot->event, hipEventDisableTiming) != hipSuccess) {
            slot->event = nullptr;
            slot->live = false;
            return check_hip(hipErrorOutOfMemory, fn, "hipEventCreate");
        }
        rc = check_hip(hipEventRecord(slot->event, s_solve), fn, "hipEventRecord");
        slot->st = st;
        slot->solve = s_solve;
        slot->live = (rc == 0);
        slot->age = ++sd.clock;
        for (int i = 0; i < 6; ++i) slot->buf[i] = mine[i];
    }
    return rc;
}

template int block_posterior_typed<double>(const void*, int64_t, int, const void*, int, const void*, int64_t, double, double, double,
                                           void*, int64_t, void*, int32_t*, void*, int64_t, void*, void*, void*, void*, void*, int, int,
                                           hipStream_t, hipStream_t, hipStream_t);
template int block_posterior_typed<float>(const void*, int64_t, int, const void*, int, const void*, int64_t, double, double, double,
                                          void*, int64_t, void*, int32_t*, void*, int64_t, void*, void*, void*, void*, void*, int, int,
                                          hipStream_t, hipStream_t, hipStream_t);

}  // namespace cimrgp
