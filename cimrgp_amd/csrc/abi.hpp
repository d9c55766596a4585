// What an extern "C" entry point needs between its arguments and its *_run call: the stream and dtype helpers, the one
// run-time -> compile-time dispatch over the dtype, and the two buffer checks that recur verbatim.
#pragma once
#include "common.hpp"

namespace cimrgp {

static inline hipStream_t stream_of(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool dtype_known(int dtype) { return dtype == CIMRGP_F32 || dtype == CIMRGP_F64; }
// (anything that is not CIMRGP_F64 counts as FP32 here: the size queries accept any dtype, the entry points check
// dtype_known or end in with_dtype)
static inline size_t elem_bytes(int dtype) { return dtype == CIMRGP_F64 ? 8 : 4; }
static inline int64_t elems_per_16_bytes(int dtype) { return dtype == CIMRGP_F64 ? 2 : 4; }

// f(float()) or f(double()) for the id `dtype`: the typed call is written once, in a generic lambda that starts with
// `using T = decltype(tag);`.  Any other id is refused in the name of the entry point `fn`.
template <typename F> static inline int with_dtype(int dtype, const char* fn, F&& f)
{
    switch (dtype) {
        case CIMRGP_F32: return f(float());
        case CIMRGP_F64: return f(double());
        default: return fail(fn, "unknown dtype");
    }
}

// a batch's blocks of `rows` rows of pitch `ld`, `cols` of them used, do not overlap at `stride` elements apart
static inline bool block_stride_ok(int64_t stride, int64_t rows, int64_t cols, int64_t ld) { return stride >= rows * ld - (ld - cols); }
// a batch's factorisation workspaces at `stride_bytes` apart: room for cimrgp_potrf_workspace_bytes, 16-byte aligned
static inline bool workspace_stride_ok(int dtype, int64_t n, size_t stride_bytes)
{
    return stride_bytes >= cimrgp_potrf_workspace_bytes(dtype, n) && stride_bytes % 16 == 0;
}

}  // namespace cimrgp
