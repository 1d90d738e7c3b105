// block_scan.h — scans and reductions inside a workgroup, each written once.  Device code only; one wave is 64 lanes.
//
// An Op is a struct with a value type T, the identity id() and an associative comb(earlier, later); WinSegMax (window_kernels.hip) shows
// that a segmented scan is just another Op.  A T that is not u32 / u64 brings its own shfl_up overload next to its Op.
//
// Two layers:
//   wave   wave_scan_inclusive, wave_reduce_all, shfl_up / shfl_xor / shfl_lane: shuffles only, no LDS and no barrier.  A hot kernel with
//          its own LDS layout and barrier choreography (the partition tiles, the scatter tile, the join chain emit, the delta decoder)
//          takes these and keeps its own wave-total write, barrier and cross-wave sum.
//   block  block_scan_exclusive, block_reduce, block_scan_array: the wave layer plus one LDS slot per wave and their own barriers, for a
//          kernel that wants the whole-workgroup answer in one call.  blockDim.x is a multiple of 64 and at most 1024 (1-D blocks).
#pragma once

#include "chgpu_internal.h"

struct AddU32 { typedef u32 T; static __device__ __forceinline__ T id() { return 0; } static __device__ __forceinline__ T comb(T a, T b) { return a + b; } };
struct AddU64 { typedef u64 T; static __device__ __forceinline__ T id() { return 0; } static __device__ __forceinline__ T comb(T a, T b) { return a + b; } };
struct MaxU32 { typedef u32 T; static __device__ __forceinline__ T id() { return 0; } static __device__ __forceinline__ T comb(T a, T b) { return a > b ? a : b; } };
struct MinU32 { typedef u32 T; static __device__ __forceinline__ T id() { return ~0u; } static __device__ __forceinline__ T comb(T a, T b) { return a < b ? a : b; } };
struct MaxU64 { typedef u64 T; static __device__ __forceinline__ T id() { return 0; } static __device__ __forceinline__ T comb(T a, T b) { return a > b ? a : b; } };
struct MinU64 { typedef u64 T; static __device__ __forceinline__ T id() { return ~0ull; } static __device__ __forceinline__ T comb(T a, T b) { return a < b ? a : b; } };
struct OrU32 { typedef u32 T; static __device__ __forceinline__ T id() { return 0; } static __device__ __forceinline__ T comb(T a, T b) { return a | b; } };

// ---------------------------------------------------------------------------------------------
// wave layer
// ---------------------------------------------------------------------------------------------
// the value of the lane d below / of the lane whose number differs in the bits of d / of lane `src`; a 64-bit value travels as two halves
__device__ __forceinline__ u32 shfl_up(u32 v, int d) { return __shfl_up(v, d, WAVE); }
__device__ __forceinline__ u64 shfl_up(u64 v, int d) { return ((u64)__shfl_up((u32)(v >> 32), d, WAVE) << 32) | __shfl_up((u32)v, d, WAVE); }
__device__ __forceinline__ u32 shfl_xor(u32 v, int d) { return __shfl_xor(v, d, WAVE); }
__device__ __forceinline__ u64 shfl_xor(u64 v, int d) { return ((u64)__shfl_xor((u32)(v >> 32), d, WAVE) << 32) | __shfl_xor((u32)v, d, WAVE); }
__device__ __forceinline__ u32 shfl_lane(u32 v, int src) { return __shfl(v, src, WAVE); }
__device__ __forceinline__ u64 shfl_lane(u64 v, int src) { return ((u64)__shfl((u32)(v >> 32), src, WAVE) << 32) | __shfl((u32)v, src, WAVE); }

// Hillis-Steele over the 64 lanes: lane i gets comb over lanes 0 .. i.  `lane` is this thread's lane number, however the caller has it.
template <typename Op>
__device__ __forceinline__ typename Op::T wave_scan_inclusive(typename Op::T v, u32 lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const typename Op::T o = shfl_up(v, d);
        if (lane >= (u32)d)
            v = Op::comb(o, v);
    }
    return v;
}
template <typename Op>
__device__ __forceinline__ typename Op::T wave_scan_inclusive(typename Op::T v)
{
    return wave_scan_inclusive<Op>(v, threadIdx.x & 63);
}

// butterfly: comb over the wave, in every lane (Op commutative)
template <typename Op>
__device__ __forceinline__ typename Op::T wave_reduce_all(typename Op::T v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = Op::comb(v, shfl_xor(v, d));
    return v;
}

// ---------------------------------------------------------------------------------------------
// block layer
// ---------------------------------------------------------------------------------------------
// Exclusive scan of one value per thread over the workgroup, in thread order.  Returns the combination of the values of all threads
// before this one; *total (when given) is the combination of all.  lds: one T per wave; may be the lds of an earlier call.
template <typename Op>
__device__ __forceinline__ typename Op::T block_scan_exclusive(typename Op::T v, typename Op::T * lds, typename Op::T * total = nullptr)
{
    typedef typename Op::T T;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const T inc = wave_scan_inclusive<Op>(v, lane);
    T exc = shfl_up(inc, 1);
    if (lane == 0)
        exc = Op::id();
    __syncthreads(); // (lds may still be read by an earlier call)
    if (lane == 63)
        lds[wave] = inc;
    __syncthreads();
    T before = Op::id();
    for (u32 w = 0; w < wave; ++w)
        before = Op::comb(before, lds[w]);
    if (total)
    {
        T all = before;
        for (u32 w = wave; w < n_waves; ++w)
            all = Op::comb(all, lds[w]);
        *total = all;
    }
    return Op::comb(before, exc);
}

// comb over the workgroup, in every thread (Op commutative).  lds: one T per wave, free again when the call returns.
template <typename Op>
__device__ __forceinline__ typename Op::T block_reduce(typename Op::T v, typename Op::T * lds)
{
    typedef typename Op::T T;
    v = wave_reduce_all<Op>(v);
    if ((threadIdx.x & 63) == 0)
        lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const u32 n_waves = blockDim.x >> 6;
    T r = lds[0];
    for (u32 w = 1; w < n_waves; ++w)
        r = Op::comb(r, lds[w]);
    __syncthreads();
    return r;
}

// One workgroup: in[0 .. n) -> out[j] = comb(first, in[0 .. j)) (REVERSE: of in(j .. n), taken from the far end), blockDim.x elements a
// pass, the carry of the passes in LDS.  Returns comb(first, all of in) in every thread.  out may be in; In may be narrower than Op::T.
template <typename Op, bool REVERSE, typename In>
__device__ __forceinline__ typename Op::T block_scan_array(const In * in, typename Op::T * out, u64 n, typename Op::T first)
{
    typedef typename Op::T T;
    __shared__ T lds[16];
    __shared__ T carry_s;
    __syncthreads();
    if (threadIdx.x == 0)
        carry_s = first;
    __syncthreads();
    for (u64 base = 0; base < n; base += blockDim.x)
    {
        const u64 q = base + threadIdx.x;
        const u64 j = REVERSE ? n - 1 - q : q;
        const T v = q < n ? (T)in[j] : Op::id();
        T total;
        const T exc = block_scan_exclusive<Op>(v, lds, &total);
        const T carry = carry_s;
        if (q < n)
            out[j] = Op::comb(carry, exc);
        __syncthreads();
        if (threadIdx.x == 0)
            carry_s = Op::comb(carry, total);
        __syncthreads();
    }
    return carry_s;
}
