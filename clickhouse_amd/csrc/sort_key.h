// sort_key.h — a column value as an order-preserving unsigned key of the same width: what the radix sort (sort_kernels.hip) splits by
// and what the merge of sorted runs (merge_kernels.hip) compares, so that both define ONE order.  Sign flip for signed integers; the IEEE
// total-order fold for floats with -0.0 and NaN canonicalised (less_stable compares with ==; NaN above or below every number by
// nan_direction_hint), so two keys are equal exactly when compareAt answers 0.  Device code only.
#pragma once

#include "chgpu_internal.h"

template <typename T>
struct SortKey;
template <> struct SortKey<u8> { typedef u8 K; static __device__ K key(u8 v, int) { return v; } };
template <> struct SortKey<u16> { typedef u16 K; static __device__ K key(u16 v, int) { return v; } };
template <> struct SortKey<u32> { typedef u32 K; static __device__ K key(u32 v, int) { return v; } };
template <> struct SortKey<u64> { typedef u64 K; static __device__ K key(u64 v, int) { return v; } };
template <> struct SortKey<i8> { typedef u8 K; static __device__ K key(i8 v, int) { return (u8)v ^ 0x80u; } };
template <> struct SortKey<i16> { typedef u16 K; static __device__ K key(i16 v, int) { return (u16)v ^ 0x8000u; } };
template <> struct SortKey<i32> { typedef u32 K; static __device__ K key(i32 v, int) { return (u32)v ^ 0x80000000u; } };
template <> struct SortKey<i64> { typedef u64 K; static __device__ K key(i64 v, int) { return (u64)v ^ 0x8000000000000000ull; } };
template <> struct SortKey<float>
{
    typedef u32 K;
    static __device__ K key(float v, int nan_hint)
    {
        if (v != v)
            return nan_hint > 0 ? 0xFFFFFFFFu : 0u;
        if (v == 0.0f)
            v = 0.0f; // -0.0 == 0.0 (less_stable compares with ==)
        const u32 b = __float_as_uint(v);
        const u32 k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        // keep the extremes free for NaN: -inf folds to 0x007FFFFF, +inf to 0xFF800000 -- neither is 0 nor all-ones
        return k;
    }
};
template <> struct SortKey<double>
{
    typedef u64 K;
    static __device__ K key(double v, int nan_hint)
    {
        if (v != v)
            return nan_hint > 0 ? ~0ull : 0ull;
        if (v == 0.0)
            v = 0.0;
        const u64 b = (u64)__double_as_longlong(v);
        return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    }
};
