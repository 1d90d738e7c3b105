// merge_keys.h — what merge_kernels.hip shares with the operators that sit on its merged order (merge_fold_kernels.hip): the sort
// description as the kernels take it, a key column's order word, and the host entry to the merged order itself (the block minimum of the
// "lowest offending row" checks is block_scan.h's block_reduce<MinU64>).  Device code except for the declarations at the end.
#pragma once

#include "block_scan.h"
#include "merge_host.h"
#include "pair_pool.h"
#include "sort_key.h"

struct MergeKeys
{
    const void * data[MRG_MAX_KEYS];
    i32 type[MRG_MAX_KEYS];
    i32 desc[MRG_MAX_KEYS];
    i32 hint[MRG_MAX_KEYS];
    u32 n;
};

template <typename T>
__device__ __forceinline__ u64 mrg_key_of(const void * data, u64 row, int desc, int hint)
{
    typedef typename SortKey<T>::K K;
    const K k = SortKey<T>::key(((const T *)data)[row], hint);
    return (u64)(desc ? (K)~k : k); // the complement inside the key's width, as k_sort_keys takes it
}

// column j of `keys` at `row` as a u64 word that orders like the column does under its description
__device__ __forceinline__ u64 mrg_key(const MergeKeys & keys, u32 j, u64 row)
{
    const void * d = keys.data[j];
    const int desc = keys.desc[j], hint = keys.hint[j];
    switch (keys.type[j])
    {
        case CHGPU_I64: return mrg_key_of<i64>(d, row, desc, hint);
        case CHGPU_U64: return mrg_key_of<u64>(d, row, desc, hint);
        case CHGPU_I32: return mrg_key_of<i32>(d, row, desc, hint);
        case CHGPU_U32: return mrg_key_of<u32>(d, row, desc, hint);
        case CHGPU_I16: return mrg_key_of<i16>(d, row, desc, hint);
        case CHGPU_U16: return mrg_key_of<u16>(d, row, desc, hint);
        case CHGPU_I8: return mrg_key_of<i8>(d, row, desc, hint);
        case CHGPU_U8: return mrg_key_of<u8>(d, row, desc, hint);
        case CHGPU_F64: return mrg_key_of<double>(d, row, desc, hint);
        default: return mrg_key_of<float>(d, row, desc, hint);
    }
}

// ---- merge_kernels.hip, for the operators over the merged order ----
// The arguments every merge entry point shares, checked in front of the device: *keys and *rows filled, or the error.
int merge_validate(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, u32 n_keys,
                   const uint64_t * run_offsets, u32 n_runs, MergeKeys * keys, u64 * rows);
// CHGPU_MERGE_CHECK_SORTED: BAD_ARGUMENTS naming the row when a run is not sorted (rows >= 2)
int merge_require_sorted(chgpu_ctx * ctx, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows);
// The merged order M of validated runs (rows >= 1, n_runs >= 1, no limit) as the merge tree's last-round arrays: words[i] is the first key
// column's order word of the row at position i of M and row_numbers[i] its concatenated row number.  The plan is merge_plan's; where it
// picks the sort chain (and for a single run) the arrays are built from the permutation.  Both live in `tmp`.
int merge_order(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, PairTemps & tmp,
                const u64 ** words, const u32 ** row_numbers);
// partial[n] -> out[0] = the minimum, by one workgroup (k_merge_min): one launch, counted
void merge_lowest(chgpu_ctx * ctx, const u64 * partial, u32 n, u64 * out);

// ---- merge_fold_kernels.hip, for the further operator over its groups (merge_versioned_kernels.hip) ----
struct FoldPrefix
{
    MergeKeys keys;
    u64 rows = 0;
};
// the argument prefix every folding merge shares, in front of the device
int fold_validate(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, u32 n_keys,
                  const uint64_t * run_offsets, u32 n_runs, u32 flags, FoldPrefix * px);
int fold_check_column(const chgpu_col * c, const char * what, int want_type, const char * type_name, u64 rows);
// BAD_ARGUMENTS naming the lowest concatenated row whose value is outside the column's domain (mode 0: Int8 sign, 1: UInt8 is_deleted)
int fold_require_domain(chgpu_ctx * ctx, PairTemps & tmp, const chgpu_col * c, int mode, u64 rows);
// heads[p] = position p of M starts a group (k_fold_heads): one launch, counted
void fold_heads(chgpu_ctx * ctx, const MergeKeys & keys, const u64 * words, const u32 * rows, u32 n, u8 * heads);
