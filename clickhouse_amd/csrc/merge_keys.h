// merge_keys.h — what merge_kernels.hip shares with the operators that sit on its merged order (merge_fold_kernels.hip,
// merge_versioned_kernels.hip), each part written once: the sort description as the kernels take it and a key column's
// order word; the tail of an emit kernel (fold_store_staged); the host entries to the merged order, to the "lowest offending row" of a
// check and to the flag check; and FoldCall, the call frame of an operator over the merged order, with the offsets step every such
// operator ends its counting with.  (The block minimum of the lowest-row checks is block_scan.h's block_reduce<MinU64>.)
#pragma once

#include <functional>

#include "block_scan.h"
#include "merge_fold_host.h"
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

// The tail of an emit kernel (k_fold_apply's emit arm, k_vc_emit): the tile's `total` staged u32 row numbers go out as u64 at
// out + base, a thread a stride, so that the stores are coalesced.  barrier: the staging writes of the workgroup are waited for first
// (a PAIRED fold stores its second column behind the same barrier).
__device__ __forceinline__ void fold_store_staged(const u32 * stage, u32 total, u64 * __restrict__ out, u64 base, bool barrier)
{
    if (barrier)
        __syncthreads();
    for (u32 e = threadIdx.x; e < total; e += FOLD_THREADS)
        out[base + e] = stage[e];
}

// ---- merge_kernels.hip, for the operators over the merged order ----
// The arguments every merge entry point shares, checked in front of the device: *keys and *rows filled, or the error.
int merge_validate(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, u32 n_keys,
                   const uint64_t * run_offsets, u32 n_runs, MergeKeys * keys, u64 * rows);
// BAD_ARGUMENTS for a flag bit other than CHGPU_MERGE_CHECK_SORTED
int merge_check_flags(u32 flags);
// CHGPU_MERGE_CHECK_SORTED: BAD_ARGUMENTS naming the row when a run is not sorted (rows >= 2)
int merge_require_sorted(chgpu_ctx * ctx, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows);
// The merged order M of validated runs (rows >= 1, n_runs >= 1, no limit) as the merge tree's last-round arrays: words[i] is the first key
// column's order word of the row at position i of M and row_numbers[i] its concatenated row number.  The plan is merge_plan's; where it
// picks the sort chain (and for a single run) the arrays are built from the permutation.  Both live in `tmp`.
int merge_order(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, PairTemps & tmp,
                const u64 ** words, const u32 ** row_numbers);
// The lowest offending row of a check over `tiles` tiles: launch_tiles(partial) launches the check's tile kernel, which leaves every
// tile's lowest offending row (~0: none) in partial[0 .. tiles); one workgroup folds them (k_merge_min) and *lowest is read back.  Two
// launches, counted here.
int merge_lowest_row(chgpu_ctx * ctx, PairTemps & tmp, u32 tiles, const std::function<void(u64 * partial)> & launch_tiles, u64 * lowest);

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

// The call frame of an operator over the merged order, behind fold_validate and the entry point's own argument checks.  It owns the
// call's allocations; `op` names the operator in the error texts.
struct FoldCall
{
    PairAllocs mem;
    PairTemps tmp{mem};         // the call's temporaries: the operator allocates its own from here
    const u64 * words = nullptr;  // M (merge_order)
    const u32 * rows = nullptr;
    u8 * heads = nullptr;       // heads[p] = position p of M starts a group
    u32 tiles = 0;              // FOLD_TILE positions each

    FoldCall(chgpu_ctx * ctx, const char * op)
    {
        mem.ctx = ctx, mem.op = op;
        mem.begin_call();
    }
    FoldCall(const FoldCall &) = delete;
    // tiles is set; for px.rows >= 1, in this order on the stream: the sorted check when the flags ask for it, the domain check of
    // domain[0 .. n_domain) (mode 0: an Int8 sign is +1 or -1, mode 1: a UInt8 is_deleted is 0 or 1; BAD_ARGUMENTS naming the lowest
    // concatenated row outside), merge_order, and the heads (k_fold_heads)
    int open(const chgpu_col * const * key_cols, const FoldPrefix & px, const uint64_t * run_offsets, u32 n_runs, u32 flags, const chgpu_col * const * domain,
             const int * domain_mode, u32 n_domain);
    // The end of the call: rc is its state so far.  A launch error turns into DEVICE under the operator's name; on any failure the
    // output columns that were made (outs[i] != NULL) are freed and their entries cleared.
    int close(int rc, chgpu_col ** outs, u32 n_outs);
};
// The step behind the tile counts (k_fold_offsets, one launch, counted): *tile_off[t] = counts[0] + .. + counts[t - 1], in `tmp`; read
// back, result[0] = the total and, only when tile_max is given, result[1] = the greatest of tile_max[0 .. tiles)
int fold_offsets(chgpu_ctx * ctx, PairTemps & tmp, const u32 * counts, const u64 * tile_max, u32 tiles, const u64 ** tile_off, u64 * result);
