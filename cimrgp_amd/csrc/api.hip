// extern "C" entry points of libcimrgp.so (declared in include/cimrgp.h and cimrgp_objective.h): checks, then with_dtype.
// The staged call behind cimrgp_block_posterior is in block.hip.
#include "abi.hpp"

#include <string.h>
#include <stdlib.h>
#include <atomic>

namespace cimrgp {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(const char* fn, const char* what)
{
    g_last_error = std::string(fn) + ": " + what;
    return -1;
}

int check_hip(hipError_t e, const char* fn, const char* what)
{
    if (e == hipSuccess) return 0;
    g_last_error = std::string(fn) + ": " + what + ": " + hipGetErrorString(e);
    return -2;
}

// ---- knobs (common.hpp) ----
const Knobs& knobs()
{
    static const Knobs k = [] {
        Knobs v;
#ifdef CIMRGP_TUNING
        auto num = [](const char* name, int64_t dflt) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : dflt; };
        v.tail_below = num("CIMRGP_TAIL_BELOW", v.tail_below);
        v.rows_start_below = num("CIMRGP_ROWS_START", v.rows_start_below);
        v.rows_start_below_early = num("CIMRGP_ROWS_START_EARLY", v.rows_start_below_early);
        v.far_pair_above = num("CIMRGP_FAR_PAIR", v.far_pair_above);
        v.gemm_pers = (int)num("CIMRGP_GEMM_PERS", v.gemm_pers);
        v.pers_min_tiles = (int)num("CIMRGP_PERS_MIN_TILES", v.pers_min_tiles);
        v.chain_cus = (int)num("CIMRGP_CHAIN_CUS", v.chain_cus);
        v.pers_max_chunks = (int)num("CIMRGP_PERS_CHUNKS", v.pers_max_chunks);
        v.early_panels = (int)num("CIMRGP_EARLY_PANELS", v.early_panels);
        v.early_cus = (int)num("CIMRGP_EARLY_CUS", v.early_cus);
        v.rows_pair_above = num("CIMRGP_ROWS_PAIR", v.rows_pair_above);
        v.fused_max_chain_wgs = num("CIMRGP_FUSED_MAX", v.fused_max_chain_wgs);
        v.batch_halves_min = (int)num("CIMRGP_BATCH_HALVES", v.batch_halves_min);
        v.rows_cus = (int)num("CIMRGP_ROWS_CUS", v.rows_cus);
        v.rider_round_us = (int)num("CIMRGP_RIDER_ROUND", v.rider_round_us);
        v.rows_beside_tail_below = num("CIMRGP_ROWS_BESIDE", v.rows_beside_tail_below);
        v.tail_far_cus = (int)num("CIMRGP_TAIL_FAR_CUS", v.tail_far_cus);
        v.tail_far_min_rows = num("CIMRGP_TAIL_FAR_MIN", v.tail_far_min_rows);
#endif
        return v;
    }();
    return k;
}

static std::atomic<int> g_rows_queues{2};
int rows_queues() { return g_rows_queues.load(std::memory_order_relaxed); }

}  // namespace cimrgp


using namespace cimrgp;

// The RBF entry points and their _cov twins share one body each: the RBF one forwards CIMRGP_COV_RBF, for which the
// covariance check is always true; `fn` names the entry point that was called in every message.  The _lin twins
// (include/cimrgp_sparse_linear.h) pass lin_entry and their weights lin_dev, which must then be there.
static int gram_impl(const char* fn, int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2, double diag_add,
                     void* k_dev, int64_t ldk, int lower_only, void* stream, bool lin_entry = false, const double* lin_dev = nullptr)
{
    CIMRGP_REQUIRE(x_dev && k_dev, fn, "null pointer");
    CIMRGP_REQUIRE(!lin_entry || lin_dev, fn, "null pointer (lin)");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(n >= 0, fn, "negative size");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return rbf_gram_run<T>((const T*)x_dev, n, (const T*)x_dev, n, d, ell, sf2, diag_add, (T*)k_dev, ldk, true, lower_only != 0,
                               stream_of(stream), cov, fn, lin_dev);
    });
}

static int cross_impl(const char* fn, int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d,
                      double ell, double sf2, void* kab_dev, int64_t ld, void* stream, bool lin_entry = false,
                      const double* lin_dev = nullptr)
{
    CIMRGP_REQUIRE(xa_dev && xb_dev && kab_dev, fn, "null pointer");
    CIMRGP_REQUIRE(!lin_entry || lin_dev, fn, "null pointer (lin)");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(na >= 0 && nb >= 0, fn, "negative size");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return rbf_gram_run<T>((const T*)xa_dev, na, (const T*)xb_dev, nb, d, ell, sf2, 0.0, (T*)kab_dev, ld, false, false,
                               stream_of(stream), cov, fn, lin_dev);
    });
}

static int predict_mean_impl(const char* fn, int dtype, int cov, const void* x_dev, int64_t n, int d, const void* alpha_dev, int q,
                             const void* xs_dev, int64_t ns, double ell, double sf2, const void* bias_dev, void* mean_dev,
                             int accumulate, void* stream)
{
    CIMRGP_REQUIRE(x_dev && alpha_dev && xs_dev && mean_dev, fn, "null pointer");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(n >= 0 && ns >= 0, fn, "negative size");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return predict_mean_run<T>((const T*)x_dev, n, d, (const T*)alpha_dev, q, (const T*)xs_dev, ns, ell, sf2, (const T*)bias_dev,
                                   (T*)mean_dev, accumulate, stream_of(stream), cov, fn);
    });
}

// cimrgp_lml_grad[_ard] and cimrgp_cov_lml_grad[_ard]; ard: pre-scaled inputs, unit length-scale.  The RBF pair
// (cov_entry false) differs from its twins in two refusals, both kept: it has never refused a length-scale <= 0 (its
// gradient is then NaN), and lml_grad_run's own messages name cimrgp_lml_grad for both of them (no name passed on).
static int lml_grad_impl(const char* fn, bool cov_entry, int dtype, int cov, bool ard, const void* x_dev, int64_t n, int d,
                         const void* kinv_dev, int64_t ldk, const void* alpha_dev, int q, double ell, double sf2, double noise,
                         double* out_dev, double* scratch_dev, void* stream)
{
    CIMRGP_REQUIRE(x_dev && kinv_dev && alpha_dev && out_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(ldk >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(!cov_entry || ell > 0.0, fn, "length-scale must be positive");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return lml_grad_run<T>((const T*)x_dev, n, d, (const T*)kinv_dev, ldk, (const T*)alpha_dev, q, ell, sf2, noise, out_dev,
                               scratch_dev, stream_of(stream), ard, cov, cov_entry ? fn : nullptr);
    });
}

// cimrgp_layer_fit[_cov] and cimrgp_layer_predict[_cov] (the _cov ones check the covariance before anything else)
static int layer_fit_impl(const char* fn, int dtype, int cov, const void* x_dev, const void* y_dev, const void* fbar_dev,
                          void* train_out_dev, const int64_t* starts_dev, int batch, int64_t n, int d, int q, double ell, double sf2,
                          double noise_fixed, double noise_frac, double noise_floor, const void* shared_bias_dev,
                          const void* shared_noise_dev, void* k_arena_dev, int64_t ldk, int64_t k_stride, void* ws_arena_dev,
                          size_t ws_stride_bytes, int32_t* info_dev, void* rows_arena_dev, int64_t ldr, void* z_dev, void* alpha_dev,
                          void* bias_dev, void* noise_dev, void* scratch_dev, void* stream)
{
    CIMRGP_REQUIRE(x_dev && y_dev && train_out_dev && starts_dev && k_arena_dev && ws_arena_dev && info_dev && rows_arena_dev &&
                   z_dev && alpha_dev && bias_dev && noise_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(batch >= 1 && n >= 1 && ldk >= n && ldr >= n, fn, "bad dimensions");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldk % e == 0 && ldr % e == 0 && k_stride % e == 0, fn, "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(block_stride_ok(k_stride, n, n, ldk), fn, "matrix stride too small");
    CIMRGP_REQUIRE(aligned16(k_arena_dev) && aligned16(ws_arena_dev) && aligned16(rows_arena_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_stride_ok(dtype, n, ws_stride_bytes), fn, "workspace stride too small or misaligned");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0, fn, "kernel parameters must be positive");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerFit<T> a;
        FitFront<T>& fr = a.fr;
        fr.bc = BatchCov{batch, d, cov, ell, sf2};
        fr.tr = Points<T>{(const T*)x_dev, starts_dev, n};
        fr.f = Factors<T>{{(T*)k_arena_dev, ldk, k_stride}, (T*)ws_arena_dev, (int64_t)(ws_stride_bytes / sizeof(T))};
        fr.info = info_dev;
        fr.y = (const T*)y_dev; fr.fbar = (const T*)fbar_dev; fr.q = q; fr.shared_bias = (const T*)shared_bias_dev;
        fr.noise_fixed = noise_fixed; fr.noise_frac = noise_frac; fr.noise_floor = noise_floor; fr.shared_noise = (const T*)shared_noise_dev;
        fr.rows = Arena<T>{(T*)rows_arena_dev, ldr, (int64_t)q * ldr};
        fr.z = (T*)z_dev; fr.alpha = (T*)alpha_dev; fr.work = (T*)scratch_dev; fr.bias = (T*)bias_dev; fr.noise = (T*)noise_dev;
        a.train_out = (T*)train_out_dev;
        return layer_fit_run<T>(a, stream_of(stream));
    });
}

static int layer_predict_impl(const char* fn, int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d,
                              const void* xs_dev, const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2,
                              const void* l_arena_dev, int64_t ldl, int64_t l_stride, const void* ws_arena_dev,
                              size_t ws_stride_bytes, const void* z_dev, int q, const void* bias_dev, const void* noise_dev,
                              void* w_arena_dev, int64_t ldw, int64_t w_stride, void* mean_dev, void* var_dev, void* stream)
{
    CIMRGP_REQUIRE(x_dev && starts_dev && xs_dev && t_starts_dev && l_arena_dev && ws_arena_dev && z_dev && w_arena_dev &&
                   mean_dev && var_dev, fn, "null pointer");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(batch >= 1 && n >= 0 && ns >= 0 && ldl >= n && ldw >= n, fn, "bad dimensions");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldw % e == 0 && l_stride % e == 0 && w_stride % e == 0, fn,
                   "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(block_stride_ok(w_stride, ns, n, ldw), fn, "W stride too small");
    CIMRGP_REQUIRE(aligned16(l_arena_dev) && aligned16(ws_arena_dev) && aligned16(w_arena_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(ws_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace stride too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerPredict<T> a;
        a.bc = BatchCov{batch, d, cov, ell, sf2};
        a.tr = Points<T>{(const T*)x_dev, starts_dev, n};
        a.te = Points<T>{(const T*)xs_dev, t_starts_dev, ns};
        a.f = Factors<const T>{{(const T*)l_arena_dev, ldl, l_stride}, (const T*)ws_arena_dev, (int64_t)(ws_stride_bytes / sizeof(T))};
        a.z = (const T*)z_dev; a.q = q; a.bias = (const T*)bias_dev; a.noise = (const T*)noise_dev;
        a.w = Arena<T>{(T*)w_arena_dev, ldw, w_stride}; a.mean = (T*)mean_dev; a.var = (T*)var_dev;
        return layer_predict_run<T>(a, stream_of(stream));
    });
}

extern "C" {

int cimrgp_version(void) { return 100; }

const char* cimrgp_last_error(void) { return g_last_error.c_str(); }

int cimrgp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cimrgp_rbf_gram(int dtype, const void* x_dev, int64_t n, int d, double ell, double sf2, double diag_add,
                    void* k_dev, int64_t ldk, int lower_only, void* stream)
{
    return gram_impl("cimrgp_rbf_gram", dtype, CIMRGP_COV_RBF, x_dev, n, d, ell, sf2, diag_add, k_dev, ldk, lower_only, stream);
}

int cimrgp_cov_gram(int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2, double diag_add,
                    void* k_dev, int64_t ldk, int lower_only, void* stream)
{
    return gram_impl("cimrgp_cov_gram", dtype, cov, x_dev, n, d, ell, sf2, diag_add, k_dev, ldk, lower_only, stream);
}

int cimrgp_rbf_cross(int dtype, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, double ell,
                     double sf2, void* kab_dev, int64_t ld, void* stream)
{
    return cross_impl("cimrgp_rbf_cross", dtype, CIMRGP_COV_RBF, xa_dev, na, xb_dev, nb, d, ell, sf2, kab_dev, ld, stream);
}

int cimrgp_cov_cross(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, double ell,
                     double sf2, void* kab_dev, int64_t ld, void* stream)
{
    return cross_impl("cimrgp_cov_cross", dtype, cov, xa_dev, na, xb_dev, nb, d, ell, sf2, kab_dev, ld, stream);
}

int cimrgp_cov_gram_lin(int dtype, int cov, const void* x_dev, int64_t n, int d, double ell, double sf2, const double* lin_dev,
                        double diag_add, void* k_dev, int64_t ldk, int lower_only, void* stream)
{
    return gram_impl("cimrgp_cov_gram_lin", dtype, cov, x_dev, n, d, ell, sf2, diag_add, k_dev, ldk, lower_only, stream, true, lin_dev);
}

int cimrgp_cov_cross_lin(int dtype, int cov, const void* xa_dev, int64_t na, const void* xb_dev, int64_t nb, int d, double ell,
                         double sf2, const double* lin_dev, void* kab_dev, int64_t ld, void* stream)
{
    return cross_impl("cimrgp_cov_cross_lin", dtype, cov, xa_dev, na, xb_dev, nb, d, ell, sf2, kab_dev, ld, stream, true, lin_dev);
}

size_t cimrgp_potrf_workspace_bytes(int dtype, int64_t n)
{
    if (n <= 0) return 0;
    const int64_t slabs = (n + 63) / 64, panels = (n + CIMRGP_NB - 1) / CIMRGP_NB, pairs = (n / CIMRGP_NB) / 2;
    // 64 x 64 inverses, 256 x 256 inverses, off-diagonal blocks of the 512 x 512 inverses (pairs of full panels)
    return (size_t)(slabs * 64 * 64 + (panels + pairs) * CIMRGP_NB * CIMRGP_NB) * elem_bytes(dtype);
}

int cimrgp_potrf(int dtype, void* k_dev, int64_t n, int64_t ldk, void* workspace_dev, size_t workspace_bytes,
                 int32_t* info_dev, void* stream)
{
    const char* fn = "cimrgp_potrf";
    CIMRGP_REQUIRE(k_dev && workspace_dev && info_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && ldk >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(ldk % elems_per_16_bytes(dtype) == 0, fn, "leading dimension must be a multiple of 16 bytes");
    CIMRGP_REQUIRE(aligned16(k_dev) && aligned16(workspace_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace too small");
    if (n == 0) return check_hip(hipMemsetAsync(info_dev, 0, sizeof(int32_t), stream_of(stream)), fn, "memset");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrf_run<T>((T*)k_dev, n, ldk, (T*)workspace_dev, info_dev, nullptr, 0, 0, stream_of(stream));
    });
}

int cimrgp_potrf_rows(int dtype, void* k_dev, int64_t n, int64_t ldk, void* workspace_dev, size_t workspace_bytes,
                      int32_t* info_dev, void* b_dev, int64_t m, int64_t ldb, void* stream)
{
    const char* fn = "cimrgp_potrf_rows";
    CIMRGP_REQUIRE(k_dev && workspace_dev && info_dev && b_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && m >= 0 && ldk >= n && ldb >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldk % e == 0 && ldb % e == 0, fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(k_dev) && aligned16(workspace_dev) && aligned16(b_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace too small");
    if (n == 0) return check_hip(hipMemsetAsync(info_dev, 0, sizeof(int32_t), stream_of(stream)), fn, "memset");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrf_run<T>((T*)k_dev, n, ldk, (T*)workspace_dev, info_dev, (T*)b_dev, m, ldb, stream_of(stream));
    });
}

int cimrgp_block_posterior(int dtype, const void* x_dev, int64_t n, int d, const void* y_dev, int q, const void* xs_dev, int64_t ns,
                           double ell, double sf2, double noise, void* k_dev, int64_t ldk, void* workspace_dev,
                           size_t workspace_bytes, int32_t* info_dev, void* w_dev, int64_t ldw, void* alpha_dev, void* z_dev,
                           void* scratch_dev, void* mean_dev, void* var_dev, int add_noise, int accumulate, void* stream)
{
    return cimrgp_block_posterior_staged(dtype, x_dev, n, d, y_dev, q, xs_dev, ns, ell, sf2, noise, k_dev, ldk, workspace_dev, workspace_bytes,
                                         info_dev, w_dev, ldw, alpha_dev, z_dev, scratch_dev, mean_dev, var_dev, add_noise, accumulate,
                                         stream, stream, stream);
}

int cimrgp_solve_queue(void* stream, void** queue_out)
{
    const char* fn = "cimrgp_solve_queue";
    CIMRGP_REQUIRE(queue_out != nullptr, fn, "null pointer");
    *queue_out = (void*)cimrgp::solve_queue_for(stream_of(stream));
    return 0;
}

int cimrgp_front_queue(void* stream, void** queue_out)
{
    const char* fn = "cimrgp_front_queue";
    CIMRGP_REQUIRE(queue_out != nullptr, fn, "null pointer");
    *queue_out = (void*)cimrgp::front_queue_for(stream_of(stream));
    return 0;
}

int cimrgp_block_posterior_staged(int dtype, const void* x_dev, int64_t n, int d, const void* y_dev, int q, const void* xs_dev, int64_t ns,
                                  double ell, double sf2, double noise, void* k_dev, int64_t ldk, void* workspace_dev,
                                  size_t workspace_bytes, int32_t* info_dev, void* w_dev, int64_t ldw, void* alpha_dev, void* z_dev,
                                  void* scratch_dev, void* mean_dev, void* var_dev, int add_noise, int accumulate,
                                  void* stream_front, void* stream, void* stream_solve)
{
    const char* fn = "cimrgp_block_posterior";
    CIMRGP_REQUIRE(x_dev && y_dev && k_dev && workspace_dev && info_dev && w_dev && alpha_dev && z_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(ns == 0 || (xs_dev && mean_dev && var_dev), fn, "null pointer (test points)");
    CIMRGP_REQUIRE(n >= 1 && ns >= 0 && ldk >= n && ldw >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldk % e == 0 && ldw % e == 0, fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(k_dev) && aligned16(workspace_dev) && aligned16(w_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace too small");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return block_posterior_typed<T>(x_dev, n, d, y_dev, q, xs_dev, ns, ell, sf2, noise, k_dev, ldk, workspace_dev, info_dev, w_dev, ldw,
                                        alpha_dev, z_dev, scratch_dev, mean_dev, var_dev, add_noise, accumulate, stream_of(stream_front),
                                        stream_of(stream), stream_of(stream_solve));
    });
}

int cimrgp_potrf_rows_batched(int dtype, void* k_dev, int64_t n, int64_t ldk, int64_t k_stride, void* workspace_dev,
                              size_t workspace_stride_bytes, int32_t* info_dev, void* b_dev, int64_t m, int64_t ldb,
                              int64_t b_stride, int batch, void* stream)
{
    const char* fn = "cimrgp_potrf_rows_batched";
    CIMRGP_REQUIRE(k_dev && workspace_dev && info_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1, fn, "batch must be >= 1");
    CIMRGP_REQUIRE(n >= 0 && m >= 0 && ldk >= n && (m == 0 || (b_dev && ldb >= n)), fn, "bad dimensions");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldk % e == 0 && (m == 0 || ldb % e == 0), fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(k_dev) && aligned16(workspace_dev) && aligned16(b_dev), fn, "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(block_stride_ok(k_stride, n, n, ldk) && k_stride % e == 0, fn, "matrix stride too small or misaligned");
    CIMRGP_REQUIRE(m == 0 || (block_stride_ok(b_stride, m, n, ldb) && b_stride % e == 0), fn, "row-block stride too small or misaligned");
    CIMRGP_REQUIRE(workspace_stride_ok(dtype, n, workspace_stride_bytes), fn, "workspace stride too small or misaligned");
    if (n == 0) return check_hip(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * (size_t)batch, stream_of(stream)), fn, "memset");
    const PotrfBatch bt{batch, k_stride, (int64_t)(workspace_stride_bytes / elem_bytes(dtype)), b_stride};
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrf_batched_run<T>((T*)k_dev, n, ldk, (T*)workspace_dev, info_dev, (T*)b_dev, m, ldb, bt, stream_of(stream));
    });
}

int cimrgp_solve_lt_batched(int dtype, const void* l_dev, int64_t n, int64_t ldl, int64_t l_stride, const void* workspace_dev,
                            size_t workspace_stride_bytes, void* z_dev, int q, void* scratch_dev, int batch, void* stream)
{
    const char* fn = "cimrgp_solve_lt_batched";
    CIMRGP_REQUIRE(l_dev && workspace_dev && z_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(batch >= 1, fn, "batch must be >= 1");
    CIMRGP_REQUIRE(n >= 0 && ldl >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(workspace_stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n), fn, "workspace stride too small");
    const PotrfBatch bt{batch, l_stride, (int64_t)(workspace_stride_bytes / elem_bytes(dtype)), 0};
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrs_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)z_dev, q, nullptr, (T*)scratch_dev, true,
                            stream_of(stream), bt);
    });
}

int cimrgp_potrs(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* rhs_dev, int q,
                 void* z_dev, void* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_potrs";
    CIMRGP_REQUIRE(l_dev && workspace_dev && rhs_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && ldl >= n, fn, "bad dimensions");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrs_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)rhs_dev, q, (T*)z_dev, (T*)scratch_dev, false,
                            stream_of(stream));
    });
}

int cimrgp_solve_lt(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* z_dev, int q,
                    void* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_solve_lt";
    CIMRGP_REQUIRE(l_dev && workspace_dev && z_dev && scratch_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && ldl >= n, fn, "bad dimensions");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return potrs_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)z_dev, q, nullptr, (T*)scratch_dev, true,
                            stream_of(stream));
    });
}

int cimrgp_trsm_rows(int dtype, const void* l_dev, int64_t n, int64_t ldl, const void* workspace_dev, void* b_dev,
                     int64_t m, int64_t ldb, void* stream)
{
    const char* fn = "cimrgp_trsm_rows";
    CIMRGP_REQUIRE(l_dev && workspace_dev && b_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && m >= 0 && ldl >= n && ldb >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldl % e == 0 && ldb % e == 0, fn, "leading dimensions must be multiples of 16 bytes");
    CIMRGP_REQUIRE(aligned16(l_dev) && aligned16(b_dev) && aligned16(workspace_dev), fn, "pointers must be 16-byte aligned");
    if (n == 0 || m == 0) return 0;
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return solve_rows_run<T>((const T*)l_dev, n, ldl, (const T*)workspace_dev, (T*)b_dev, m, ldb, stream_of(stream));
    });
}

int cimrgp_predict_mean(int dtype, const void* x_dev, int64_t n, int d, const void* alpha_dev, int q, const void* xs_dev,
                        int64_t ns, double ell, double sf2, const void* bias_dev, void* mean_dev, int accumulate,
                        void* stream)
{
    return predict_mean_impl("cimrgp_predict_mean", dtype, CIMRGP_COV_RBF, x_dev, n, d, alpha_dev, q, xs_dev, ns, ell, sf2, bias_dev,
                             mean_dev, accumulate, stream);
}

int cimrgp_cov_predict_mean(int dtype, int cov, const void* x_dev, int64_t n, int d, const void* alpha_dev, int q,
                            const void* xs_dev, int64_t ns, double ell, double sf2, const void* bias_dev, void* mean_dev,
                            int accumulate, void* stream)
{
    return predict_mean_impl("cimrgp_cov_predict_mean", dtype, cov, x_dev, n, d, alpha_dev, q, xs_dev, ns, ell, sf2, bias_dev, mean_dev,
                             accumulate, stream);
}

int cimrgp_predict_from_w(int dtype, const void* w_dev, int64_t ns, int64_t n, int64_t ldw, const void* z_dev, int q,
                          double sf2, double extra_var, const void* extra_var_dev, const void* bias_dev, void* mean_dev,
                          void* var_dev, int accumulate, void* stream)
{
    const char* fn = "cimrgp_predict_from_w";
    CIMRGP_REQUIRE(w_dev, fn, "null pointer");
    CIMRGP_REQUIRE(ns >= 0 && n >= 0 && ldw >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(mean_dev == nullptr || z_dev != nullptr, fn, "mean requested without z");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return predict_from_w_run<T>((const T*)w_dev, ns, n, ldw, (const T*)z_dev, q, sf2, extra_var, (const T*)extra_var_dev,
                                     (const T*)bias_dev, (T*)mean_dev, (T*)var_dev, accumulate, stream_of(stream));
    });
}

int cimrgp_block_stats(int dtype, const void* y_dev, const void* fbar_dev, int64_t n, int q, void* stats_dev, void* stream)
{
    const char* fn = "cimrgp_block_stats";
    CIMRGP_REQUIRE(y_dev && stats_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_block_stats<T>((const T*)y_dev, (const T*)fbar_dev, n, q, (T*)stats_dev, stream_of(stream));
    });
}

int cimrgp_residual(int dtype, const void* y_dev, const void* fbar_dev, const void* bias_dev, int64_t n, int q,
                    void* r_dev, void* stream)
{
    const char* fn = "cimrgp_residual";
    CIMRGP_REQUIRE(y_dev && r_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_residual<T>((const T*)y_dev, (const T*)fbar_dev, (const T*)bias_dev, n, q, (T*)r_dev, stream_of(stream));
    });
}

int cimrgp_train_mean(int dtype, const void* r_dev, const void* alpha_dev, const void* bias_dev, const void* noise_dev,
                      int64_t n, int q, void* out_dev, int accumulate, void* stream)
{
    const char* fn = "cimrgp_train_mean";
    CIMRGP_REQUIRE(r_dev && alpha_dev && noise_dev && out_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_train_mean<T>((const T*)r_dev, (const T*)alpha_dev, (const T*)bias_dev, (const T*)noise_dev, n, q, (T*)out_dev,
                                  accumulate, stream_of(stream));
    });
}

int cimrgp_add_diag(int dtype, void* k_dev, int64_t n, int64_t ldk, const void* noise_dev, void* stream)
{
    const char* fn = "cimrgp_add_diag";
    CIMRGP_REQUIRE(k_dev && noise_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_add_diag<T>((T*)k_dev, n, ldk, (const T*)noise_dev, stream_of(stream));
    });
}

int cimrgp_noise_from_stats(int dtype, const void* stats_dev, int q, double frac, double floor_value, void* noise_dev,
                            void* stream)
{
    const char* fn = "cimrgp_noise_from_stats";
    CIMRGP_REQUIRE(stats_dev && noise_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_noise_from_stats<T>((const T*)stats_dev, q, frac, floor_value, (T*)noise_dev, stream_of(stream));
    });
}

int cimrgp_logdet_half(int dtype, const void* l_dev, int64_t n, int64_t ldl, double* out_dev, void* stream)
{
    const char* fn = "cimrgp_logdet_half";
    CIMRGP_REQUIRE(l_dev && out_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return misc_logdet_half<T>((const T*)l_dev, n, ldl, out_dev, stream_of(stream));
    });
}

int cimrgp_syrk_lower(int dtype, void* c_dev, int64_t ldc, const void* a_dev, int64_t lda, int64_t n, int64_t k, void* stream)
{
    const char* fn = "cimrgp_syrk_lower";
    CIMRGP_REQUIRE(c_dev && a_dev, fn, "null pointer");
    CIMRGP_REQUIRE(n >= 0 && k >= 0 && ldc >= n && lda >= k && k < (1ll << 31), fn, "bad dimensions");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return gemm_nt_sub<T>((T*)c_dev, ldc, (const T*)a_dev, lda, (const T*)a_dev, lda, n, n, (int)k, true, stream_of(stream));
    });
}

int cimrgp_lml_grad(int dtype, const void* x_dev, int64_t n, int d, const void* kinv_dev, int64_t ldk, const void* alpha_dev,
                    int q, double ell, double sf2, double noise, double* out_dev, double* scratch_dev, void* stream)
{
    return lml_grad_impl("cimrgp_lml_grad", false, dtype, CIMRGP_COV_RBF, false, x_dev, n, d, kinv_dev, ldk, alpha_dev, q, ell, sf2, noise,
                         out_dev, scratch_dev, stream);
}

int cimrgp_lml_grad_ard(int dtype, const void* xs_dev, int64_t n, int d, const void* kinv_dev, int64_t ldk,
                        const void* alpha_dev, int q, double sf2, double noise, double* out_dev, double* scratch_dev,
                        void* stream)
{
    return lml_grad_impl("cimrgp_lml_grad_ard", false, dtype, CIMRGP_COV_RBF, true, xs_dev, n, d, kinv_dev, ldk, alpha_dev, q, 1.0, sf2,
                         noise, out_dev, scratch_dev, stream);
}

int cimrgp_cov_lml_grad(int dtype, int cov, const void* x_dev, int64_t n, int d, const void* kinv_dev, int64_t ldk,
                        const void* alpha_dev, int q, double ell, double sf2, double noise, double* out_dev, double* scratch_dev,
                        void* stream)
{
    return lml_grad_impl("cimrgp_cov_lml_grad", true, dtype, cov, false, x_dev, n, d, kinv_dev, ldk, alpha_dev, q, ell, sf2, noise, out_dev,
                         scratch_dev, stream);
}

int cimrgp_cov_lml_grad_ard(int dtype, int cov, const void* xs_dev, int64_t n, int d, const void* kinv_dev, int64_t ldk,
                            const void* alpha_dev, int q, double sf2, double noise, double* out_dev, double* scratch_dev,
                            void* stream)
{
    return lml_grad_impl("cimrgp_cov_lml_grad_ard", true, dtype, cov, true, xs_dev, n, d, kinv_dev, ldk, alpha_dev, q, 1.0, sf2, noise,
                         out_dev, scratch_dev, stream);
}

size_t cimrgp_lml_grad_scratch_bytes(int64_t n)
{
    if (n <= 0) return 0;
    const int64_t tm = (n + 63) / 64;
    return (size_t)(tm * (tm + 1) / 2) * 10 * sizeof(double);      // 10 = the ARD record (sf | 8 dimensions | trace)
}

int cimrgp_laplace_basis(int dtype, const void* x_dev, int64_t n, int d, const double* interval_dev, int m, void* phi_dev,
                         void* stream)
{
    const char* fn = "cimrgp_laplace_basis";
    CIMRGP_REQUIRE(x_dev && interval_dev && phi_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return laplace_basis_run<T>((const T*)x_dev, n, d, interval_dev, m, (T*)phi_dev, stream_of(stream));
    });
}

size_t cimrgp_basis_moments_scratch_bytes(int64_t n, int m, int q)
{
    if (n <= 0) return 0;
    return (size_t)basis_moments_workgroups(n) * (size_t)(m * q + 2 * m + q + 2) * sizeof(double);
}

int cimrgp_basis_moments(int dtype, const void* x_dev, int64_t n, int d, const double* interval_dev, int m, const void* y_dev,
                         const void* fbar_dev, const void* fvar_dev, const double* eau_dev, int q, double* out_dev,
                         double* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_basis_moments";
    CIMRGP_REQUIRE(x_dev && interval_dev && y_dev && eau_dev && out_dev && scratch_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return basis_moments_run<T>((const T*)x_dev, n, d, interval_dev, m, (const T*)y_dev, (const T*)fbar_dev, (const T*)fvar_dev,
                                    eau_dev, q, out_dev, scratch_dev, stream_of(stream));
    });
}

int cimrgp_basis_apply(int dtype, const void* x_dev, int64_t n, int d, const double* interval_dev, int m, const double* eau_dev,
                       int q, const double* bias_dev, const double* c2_dev, double bias_var, void* mean_dev, void* var_dev,
                       int accumulate, void* stream)
{
    const char* fn = "cimrgp_basis_apply";
    CIMRGP_REQUIRE(x_dev && interval_dev && eau_dev, fn, "null pointer");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        return basis_apply_run<T>((const T*)x_dev, n, d, interval_dev, m, eau_dev, q, bias_dev, c2_dev, bias_var, (T*)mean_dev,
                                  (T*)var_dev, accumulate, stream_of(stream));
    });
}

int cimrgp_layer_fit(int dtype, const void* x_dev, const void* y_dev, const void* fbar_dev, void* train_out_dev,
                     const int64_t* starts_dev, int batch, int64_t n, int d, int q, double ell, double sf2, double noise_fixed,
                     double noise_frac, double noise_floor, const void* shared_bias_dev, const void* shared_noise_dev,
                     void* k_arena_dev, int64_t ldk, int64_t k_stride, void* ws_arena_dev, size_t ws_stride_bytes,
                     int32_t* info_dev, void* rows_arena_dev, int64_t ldr, void* z_dev, void* alpha_dev, void* bias_dev,
                     void* noise_dev, void* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_layer_fit";
    return layer_fit_impl(fn, dtype, CIMRGP_COV_RBF, x_dev, y_dev, fbar_dev, train_out_dev, starts_dev, batch, n, d, q, ell, sf2,
                          noise_fixed, noise_frac, noise_floor, shared_bias_dev, shared_noise_dev, k_arena_dev, ldk, k_stride,
                          ws_arena_dev, ws_stride_bytes, info_dev, rows_arena_dev, ldr, z_dev, alpha_dev, bias_dev, noise_dev,
                          scratch_dev, stream);
}

int cimrgp_layer_fit_cov(int dtype, int cov, const void* x_dev, const void* y_dev, const void* fbar_dev, void* train_out_dev,
                         const int64_t* starts_dev, int batch, int64_t n, int d, int q, double ell, double sf2, double noise_fixed,
                         double noise_frac, double noise_floor, const void* shared_bias_dev, const void* shared_noise_dev,
                         void* k_arena_dev, int64_t ldk, int64_t k_stride, void* ws_arena_dev, size_t ws_stride_bytes,
                         int32_t* info_dev, void* rows_arena_dev, int64_t ldr, void* z_dev, void* alpha_dev, void* bias_dev,
                         void* noise_dev, void* scratch_dev, void* stream)
{
    const char* fn = "cimrgp_layer_fit_cov";
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    return layer_fit_impl(fn, dtype, cov, x_dev, y_dev, fbar_dev, train_out_dev, starts_dev, batch, n, d, q, ell, sf2,
                          noise_fixed, noise_frac, noise_floor, shared_bias_dev, shared_noise_dev, k_arena_dev, ldk, k_stride,
                          ws_arena_dev, ws_stride_bytes, info_dev, rows_arena_dev, ldr, z_dev, alpha_dev, bias_dev, noise_dev,
                          scratch_dev, stream);
}

int cimrgp_layer_predict(int dtype, const void* x_dev, const int64_t* starts_dev, int64_t n, int d, const void* xs_dev,
                         const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2, const void* l_arena_dev,
                         int64_t ldl, int64_t l_stride, const void* ws_arena_dev, size_t ws_stride_bytes, const void* z_dev, int q,
                         const void* bias_dev, const void* noise_dev, void* w_arena_dev, int64_t ldw, int64_t w_stride,
                         void* mean_dev, void* var_dev, void* stream)
{
    const char* fn = "cimrgp_layer_predict";
    return layer_predict_impl(fn, dtype, CIMRGP_COV_RBF, x_dev, starts_dev, n, d, xs_dev, t_starts_dev, ns, batch, ell, sf2,
                              l_arena_dev, ldl, l_stride, ws_arena_dev, ws_stride_bytes, z_dev, q, bias_dev, noise_dev, w_arena_dev,
                              ldw, w_stride, mean_dev, var_dev, stream);
}

int cimrgp_layer_predict_cov(int dtype, int cov, const void* x_dev, const int64_t* starts_dev, int64_t n, int d,
                             const void* xs_dev, const int64_t* t_starts_dev, int64_t ns, int batch, double ell, double sf2,
                             const void* l_arena_dev, int64_t ldl, int64_t l_stride, const void* ws_arena_dev,
                             size_t ws_stride_bytes, const void* z_dev, int q, const void* bias_dev, const void* noise_dev,
                             void* w_arena_dev, int64_t ldw, int64_t w_stride, void* mean_dev, void* var_dev, void* stream)
{
    const char* fn = "cimrgp_layer_predict_cov";
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    return layer_predict_impl(fn, dtype, cov, x_dev, starts_dev, n, d, xs_dev, t_starts_dev, ns, batch, ell, sf2, l_arena_dev, ldl,
                              l_stride, ws_arena_dev, ws_stride_bytes, z_dev, q, bias_dev, noise_dev, w_arena_dev, ldw, w_stride,
                              mean_dev, var_dev, stream);
}

size_t cimrgp_layer_lml_grad_scratch_bytes(int dtype, int64_t n, int q, int batch)
{
    if (!dtype_known(dtype) || n <= 0 || q < 1 || batch < 1) return 0;
    return lml_scratch_layout(elem_bytes(dtype), n, q, batch, lml_grad_record_width(false)).total;
}

size_t cimrgp_layer_lml_grad_ard_scratch_bytes(int dtype, int64_t n, int q, int batch)
{
    if (!dtype_known(dtype) || n <= 0 || q < 1 || batch < 1) return 0;
    return lml_scratch_layout(elem_bytes(dtype), n, q, batch, lml_grad_record_width(true)).total;
}

// cimrgp_layer_lml_grad_cov and cimrgp_layer_lml_grad_ard_cov; ard: pre-scaled inputs, unit length-scale (ell = 1.0 passed)
static int layer_lml_grad_impl(const char* fn, bool ard, int dtype, int cov, const void* x_dev, const void* y_dev,
                               const void* fbar_dev, const int64_t* starts_dev, int batch, int64_t n, int d, int q, double ell,
                               double sf2, double noise, const void* shared_bias_dev, void* k_arena_dev, int64_t ldk,
                               int64_t k_stride, void* kinv_arena_dev, void* ws_arena_dev, size_t ws_stride_bytes,
                               int32_t* info_dev, void* scratch_dev, double* out_dev, void* stream)
{
    CIMRGP_REQUIRE(x_dev && y_dev && starts_dev && k_arena_dev && kinv_arena_dev && ws_arena_dev && info_dev && scratch_dev && out_dev,
                   fn, "null pointer");
    CIMRGP_REQUIRE(cov_known(cov), fn, "unknown covariance");
    CIMRGP_REQUIRE(dtype_known(dtype), fn, "unknown dtype");
    CIMRGP_REQUIRE(batch >= 1 && batch < 65536 && n >= 1 && n < (1ll << 30) && ldk >= n, fn, "bad dimensions");
    CIMRGP_REQUIRE(d >= 1 && d <= MAXD, fn, "input dimension must be in [1, 8]");
    CIMRGP_REQUIRE(q >= 1 && q <= MAXQ, fn, "number of outputs must be in [1, 8]");
    const int64_t e = elems_per_16_bytes(dtype);
    CIMRGP_REQUIRE(ldk % e == 0 && k_stride % e == 0, fn, "leading dimensions and strides must be multiples of 16 bytes");
    CIMRGP_REQUIRE(block_stride_ok(k_stride, n, n, ldk), fn, "matrix stride too small");
    CIMRGP_REQUIRE(aligned16(k_arena_dev) && aligned16(kinv_arena_dev) && aligned16(ws_arena_dev) && aligned16(scratch_dev), fn,
                   "pointers must be 16-byte aligned");
    CIMRGP_REQUIRE(workspace_stride_ok(dtype, n, ws_stride_bytes), fn, "workspace stride too small or misaligned");
    CIMRGP_REQUIRE(ell > 0.0 && sf2 > 0.0 && noise >= 0.0, fn, "kernel parameters must be positive (noise non-negative)");
    return with_dtype(dtype, fn, [&](auto tag) {
        using T = decltype(tag);
        LayerLml<T> a;
        FitFront<T>& fr = a.fr;
        fr.bc = BatchCov{batch, d, cov, ell, sf2};
        fr.tr = Points<T>{(const T*)x_dev, starts_dev, n};
        fr.f = Factors<T>{{(T*)k_arena_dev, ldk, k_stride}, (T*)ws_arena_dev, (int64_t)(ws_stride_bytes / sizeof(T))};
        fr.info = info_dev;
        fr.y = (const T*)y_dev; fr.fbar = (const T*)fbar_dev; fr.q = q; fr.shared_bias = (const T*)shared_bias_dev;
        fr.noise_fixed = noise;
        a.kinv = (T*)kinv_arena_dev; a.scratch = scratch_dev; a.out = out_dev;
        return layer_lml_grad_run<T>(a, stream_of(stream), ard);
    });
}

int cimrgp_layer_lml_grad_cov(int dtype, int cov, const void* x_dev, const void* y_dev, const void* fbar_dev,
                              const int64_t* starts_dev, int batch, int64_t n, int d, int q, double ell, double sf2,
                              double noise, const void* shared_bias_dev, void* k_arena_dev, int64_t ldk, int64_t k_stride,
                              void* kinv_arena_dev, void* ws_arena_dev, size_t ws_stride_bytes, int32_t* info_dev,
                              void* scratch_dev, double* out_dev, void* stream)
{
    return layer_lml_grad_impl("cimrgp_layer_lml_grad_cov", false, dtype, cov, x_dev, y_dev, fbar_dev, starts_dev, batch, n, d, q, ell,
                               sf2, noise, shared_bias_dev, k_arena_dev, ldk, k_stride, kinv_arena_dev, ws_arena_dev, ws_stride_bytes,
                               info_dev, scratch_dev, out_dev, stream);
}

int cimrgp_layer_lml_grad_ard_cov(int dtype, int cov, const void* xs_dev, const void* y_dev, const void* fbar_dev,
                                  const int64_t* starts_dev, int batch, int64_t n, int d, int q, double sf2, double noise,
                                  const void* shared_bias_dev, void* k_arena_dev, int64_t ldk, int64_t k_stride,
                                  void* kinv_arena_dev, void* ws_arena_dev, size_t ws_stride_bytes, int32_t* info_dev,
                                  void* scratch_dev, double* out_dev, void* stream)
{
    return layer_lml_grad_impl("cimrgp_layer_lml_grad_ard_cov", true, dtype, cov, xs_dev, y_dev, fbar_dev, starts_dev, batch, n, d, q,
                               1.0, sf2, noise, shared_bias_dev, k_arena_dev, ldk, k_stride, kinv_arena_dev, ws_arena_dev,
                               ws_stride_bytes, info_dev, scratch_dev, out_dev, stream);
}

int cimrgp_set_rows_queues(int queues)
{
    if (queues != 1 && queues != 2) return fail("cimrgp_set_rows_queues", "queues must be 1 or 2");
    g_rows_queues.store(queues, std::memory_order_relaxed);
    return 0;
}

int cimrgp_get_rows_queues(void) { return rows_queues(); }

int cimrgp_shutdown(void) { const int rc = potrf_shutdown(); staged_shutdown_(); return rc; }

int cimrgp_tuning_build(void)
{
#ifdef CIMRGP_TUNING
    return 1;
#else
    return 0;
#endif
}

int cimrgp_profile_begin(void) { return profile_begin(); }

int cimrgp_profile_pause(void) { return cimrgp::profile_pause(); }

int cimrgp_profile_collect(double* total_ms, double* total_flops, int64_t* launches)
{
    return profile_collect(total_ms, total_flops, launches);
}

int cimrgp_profile_collect_bytes(double* total_ms, double* total_flops, double* total_bytes, int64_t* launches)
{
    return profile_collect(total_ms, total_flops, launches, total_bytes);
}

}  // extern "C"
