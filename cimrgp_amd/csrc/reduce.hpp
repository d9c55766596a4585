// The fixed summation orders of the small row-wise and reduction kernels, each written once (device code only).
// Every sum of these kernels is one of the orders below, so a result is bit-identical on repetition, and independent of
// the launch geometry wherever the order is a function of the element's index alone.  A kernel's header comment names
// the order it uses; DESIGN.md (section 4) lists which kernel uses which.
//
// Not here: reduced.hip's lane-group combine in k_basis_moments (off = width, 2 width, .. 32, ASCENDING, with a
// run-time width = the number of basis functions rounded up to a power of two).  It adds the 64 / width lane groups of a
// wave, not the 64 lanes, and it starts from the nearest partner: for width = 1 it visits the offsets of wave_sum in
// the opposite order (1, 2, .. 32 against 32, 16, .. 1), which pairs other partial sums and rounds differently.  It is
// a different order and stays where it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace cimrgp {

// ------------------------------------------------------------- wave_sum ----
// One step of the butterfly for one value: a scalar, or a fixed-size array (of arrays) element by element.
template <typename V>
static __device__ __forceinline__ void xor_step(V& v, int off)
{
    if constexpr (std::is_array_v<V>) {
#pragma unroll
        for (int i = 0; i < (int)std::extent_v<V>; ++i) xor_step(v[i], off);
    } else {
        v += __shfl_xor(v, off, 64);
    }
}

// The xor butterfly over LANES consecutive lanes (64: the wave; 32: each half wave on its own): offsets LANES / 2,
// LANES / 4, .. 1, v += the partner's v at every step, so that every lane ends with the sum of its group in one fixed
// pairing.  Several values advance together, one step at a time in argument order, as a hand-written loop over them
// would (finishing one value before the next costs registers).
template <int LANES = 64, typename... V>
static __device__ __forceinline__ void wave_sum(V&... v)
{
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) (xor_step(v, off), ...);
}

// ------------------------------------------------------------ block_sum ----
// The sum of v over the workgroup (whole waves, at most 16): wave_sum, then the waves' lane-0 values through LDS
// (red: one element per wave), added in wave order 0, 1, ..  Every thread returns the sum.  red may be reused at once:
// the call starts with a barrier.
template <typename T>
static __device__ __forceinline__ T block_sum(T v, T* red)
{
    wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T s = (T)0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

// ------------------------------------------------------------- lds_tree ----
// The pairwise tree over the N threads of a workgroup, for C columns at once: thread t has stored its partial sum of
// column c in red[c * N + t]; then red[t] += red[t + half] for half = N / 2, N / 4, .. 1.  Column c's sum ends in
// red[c * N], visible to every thread on return.
template <int N, int C = 1>
static __device__ __forceinline__ void lds_tree(double* red, int tid)
{
    __syncthreads();
    for (int half = N / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int c = 0; c < C; ++c) red[c * N + tid] += red[c * N + tid + half];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- sum4 ----
// The four waves' partial sums of a 256-thread workgroup, in wave order.
template <typename T>
static __device__ __forceinline__ T sum4(T p0, T p1, T p2, T p3) { return ((p0 + p1) + p2) + p3; }

// ------------------------------------------------------------ row walk ----
// A wave per row, four rows per 256-thread workgroup: this wave's row and lane; false (the wave leaves) past the last
// row.  Lane l then takes columns l, l + 64, .. in FP64 (`for (int j = lane; j < m; j += 64)`), wave_sum adds the 64
// partial sums, and lane 0 writes.
template <typename I>
static __device__ __forceinline__ bool wave_row(I rows, I& row, int& lane)
{
    row = (I)blockIdx.x * 4 + (I)(threadIdx.x >> 6);
    lane = threadIdx.x & 63;
    return row < rows;
}

// acc[c] += v g[c] for c < q: one column's term of a row's dot products with the q columns of gamma (g = its row j)
template <typename T, int Q>
static __device__ __forceinline__ void dot_step(double (&acc)[Q], double v, const T* __restrict__ g, int q)
{
#pragma unroll
    for (int c = 0; c < Q; ++c)
        if (c < q) acc[c] += v * (double)g[c];
}

// *p = v, or *p += v for an accumulating call
template <typename T>
static __device__ __forceinline__ void put(T* p, T v, int accumulate) { *p = accumulate ? *p + v : v; }

// ----------------------------------------------------------- block_stats ----
// One workgroup over a block of n rows and q columns: smean[c] = the column means of y - fbar (fbar may be nullptr),
// returned: the pooled population variance about them.  Thread t takes elements t, t + blockDim.x, ..; block_sum adds.
// red: 16 elements, smean: q elements, both in LDS; smean is visible to every thread on return.
template <typename T>
static __device__ __forceinline__ T block_stats(const T* __restrict__ y, const T* __restrict__ fbar, int64_t n, int q, T* red, T* smean)
{
    for (int c = 0; c < q; ++c) {
        T s = (T)0;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x)
            s += y[i * q + c] - (fbar ? fbar[i * q + c] : (T)0);
        s = block_sum(s, red);
        if (threadIdx.x == 0) smean[c] = s / (T)n;
    }
    __syncthreads();
    T s2 = (T)0;
    for (int64_t e = threadIdx.x; e < n * q; e += blockDim.x) {
        const int c = (int)(e % q);
        const T r = y[e] - (fbar ? fbar[e] : (T)0) - smean[c];
        s2 += r * r;
    }
    return block_sum(s2, red) / (T)(n * q);
}

}  // namespace cimrgp
